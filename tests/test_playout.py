"""CPU checks of spl_playout's boundary: the header declares it, the built library exports it,
the ctypes binding lists it, and every bad argument is rejected before any launch (no device
is touched: the calls run on a machine without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splendor_amd.h")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsplendor_amd.so not built")


def test_header_declares_playout():
    src = open(HEADER).read()
    assert re.search(r"^\s*int\s+spl_playout\s*\(", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_PLAYOUT_UNIFORM\s+0\s*$", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_PLAYOUT_BUY_FIRST\s+1\s*$", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_ABI_VERSION\s+11\s*$", src, flags=re.M)     # additive: no bump


@needs_lib
def test_library_exports_playout():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "spl_playout")
    assert lib.spl_abi_version() == 11


@needs_lib
def test_binding_lists_playout():
    from splendor import _lib
    assert "spl_playout" in _lib.exported_symbols()
    args, res = _lib._SIGS["spl_playout"]
    assert len(args) == 16 and res is ctypes.c_int
    assert (_lib.PLAYOUT_UNIFORM, _lib.PLAYOUT_BUY_FIRST) == (0, 1)
    assert _lib.ABI_VERSION == 11
    from splendor.env import SplendorEngine
    assert SplendorEngine.PLAYOUT_POLICIES == {"uniform": 0, "buy_first": 1}


@needs_lib
def test_playout_argument_validation():
    """SPL_EINVAL for every argument the header rules out, and B == 0 as a no-op, all before
    any launch (the pointers are dummies that are never dereferenced)."""
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    f = lib.spl_playout
    f.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp,
                  vp, vp]
    f.restype = ci
    lib.spl_ctx_destroy.argtypes = [vp]
    h = vp()
    assert lib.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    d = vp(1)

    def call(ctx=h, B=0, state=d, policy=1, playouts=1, max_steps=124, step0=0, result=d):
        return f(ctx, B, state, None, None, policy, playouts, max_steps, 0x5EED, step0, 0, result, None, None,
                 None, None)

    assert call() == 0                                        # B == 0: nothing launched
    assert call(policy=0, playouts=64, max_steps=1024) == 0
    assert call(max_steps=1, step0=0x7FFFFFFF) == 0           # step0 + max_steps == 2^31: the last stream
    assert call(ctx=None) == -1
    assert call(state=None) == -1
    assert call(result=None) == -1
    assert call(B=-1) == -1
    assert call(B=4, state=None) == -1
    for policy in (-1, 2):
        assert call(policy=policy) == -1
    for playouts in (0, -1, 65):
        assert call(playouts=playouts) == -1
    for max_steps in (0, -1, 1025):
        assert call(max_steps=max_steps) == -1
    assert call(max_steps=2, step0=0x7FFFFFFF) == -1          # would reach the deal streams
    assert call(max_steps=124, step0=0x80000000 - 123) == -1
    assert call(max_steps=124, step0=0xFFFFFFFF) == -1        # (no uint32 wrap in the check)
    lib.spl_ctx_destroy(h)


def test_evaluator_rejects_bad_settings():
    from splendor.playout import PlayoutEvaluator
    with pytest.raises(ValueError):
        PlayoutEvaluator(None, policy="greedy")
    with pytest.raises(ValueError):
        PlayoutEvaluator(None, playouts=65)
    ev = PlayoutEvaluator(None, playouts=4, policy="uniform", seed=3, board_base=7)
    assert (ev.playouts, ev.policy, ev.seed, ev.board_base, ev.calls) == (4, "uniform", 3, 7, 0)
