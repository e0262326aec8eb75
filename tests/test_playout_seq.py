"""CPU checks of spl_playout_seq's boundary: the header declares it, the built library exports
it, the ctypes binding lists it, every bad argument is rejected before any launch (no device is
touched: the calls run on a machine without a GPU), and the evaluator still constructs without
an engine."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splendor_amd.h")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsplendor_amd.so not built")


def test_header_declares_playout_seq():
    src = open(HEADER).read()
    assert re.search(r"^\s*int\s+spl_playout_seq\s*\(", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_PLAYOUT_SEQ_STREAMS\s+256\s*$", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_ABI_VERSION\s+11\s*$", src, flags=re.M)     # additive: no bump


@needs_lib
def test_library_exports_playout_seq():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "spl_playout_seq") and hasattr(lib, "spl_playout")
    assert lib.spl_abi_version() == 11


@needs_lib
def test_binding_lists_playout_seq():
    from splendor import _lib
    assert "spl_playout_seq" in _lib.exported_symbols()
    args, res = _lib._SIGS["spl_playout_seq"]
    assert len(args) == 17 and res is ctypes.c_int
    assert _lib.ABI_VERSION == 11
    from splendor.env import SplendorEngine
    assert callable(SplendorEngine.playout_seq)


@needs_lib
def test_playout_seq_argument_validation():
    """SPL_EINVAL for every argument the header rules out, and B == 0 as a no-op, all before
    any launch (the pointers are dummies that are never dereferenced)."""
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    f = lib.spl_playout_seq
    f.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    f.restype = ci
    lib.spl_ctx_destroy.argtypes = [vp]
    h = vp()
    assert lib.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    d = vp(1)

    def call(ctx=h, B=0, state=d, active=None, index=None, count=None, policy=1, playouts=1, max_steps=124,
             seq=d, result=d):
        return f(ctx, B, state, active, index, count, policy, playouts, max_steps, 0x5EED, seq, 0, result, None,
                 None, None, None)

    assert call() == 0                                        # B == 0: nothing launched
    assert call(policy=0, playouts=64, max_steps=256) == 0
    assert call(active=d) == 0
    assert call(index=d, count=d) == 0
    assert call(max_steps=1) == 0
    assert call(ctx=None) == -1
    assert call(state=None) == -1
    assert call(result=None) == -1
    assert call(seq=None) == -1
    assert call(B=4, seq=None) == -1
    assert call(active=d, index=d, count=d) == -1             # flags together with a list
    assert call(index=d) == -1                                # half a list
    assert call(count=d) == -1
    assert call(active=d, index=d) == -1
    assert call(active=d, count=d) == -1
    for max_steps in (0, 257, 1024):
        assert call(max_steps=max_steps) == -1
    for policy in (-1, 2):
        assert call(policy=policy) == -1
    for playouts in (0, -1, 65):
        assert call(playouts=playouts) == -1
    assert call(B=-1) == -1
    lib.spl_ctx_destroy(h)


def test_evaluator_constructs_without_a_device():
    from splendor.playout import PlayoutEvaluator
    ev = PlayoutEvaluator(None, playouts=4, policy="uniform", seed=3, board_base=7)
    assert ev.calls == 0 and ev.indexed is True
    assert (ev.playouts, ev.policy, ev.seed, ev.board_base) == (4, "uniform", 3, 7)
    assert ev.calls == 0                                      # (a property: reading it allocates nothing)
