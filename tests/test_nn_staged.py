"""CPU checks of the staged leaf buffer's C ABI: spl_nn_stage_bytes against the layout
documented in include/splendor_amd.h, and the SPL_EINVAL cases of the three staged entry points
(rejected before any launch, so no device is needed). Additive: the ABI version stays 11."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splendor_amd.h")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsplendor_amd.so not built")


def a16(x):
    return (x + 15) // 16 * 16


def documented_bytes(n, B):
    """The header's layout, written out: total + reserved, rows[B] i32, mask[B][7] u64 and
    ceil(B / 32) tiles of 7 x 32 x X0S int8, the last two from 16-byte boundaries."""
    R = 32 + 10 * n + n * n
    kp = (R + 7) // 8 * 8
    x0s = kp if (kp // 4) % 2 else kp + 4
    m = a16(16 + 4 * B)
    x = a16(m + 56 * B)
    return x + (B + 31) // 32 * 7 * 32 * x0s


def test_header_declares_staged_entry_points():
    src = open(HEADER).read()
    assert re.search(r"^long long\s+spl_nn_stage_bytes\s*\(", src, flags=re.M)
    for name in ("spl_mcts_select_staged", "spl_nn_stage_leaves", "spl_nn_forward_staged"):
        assert re.search(rf"^int\s+{name}\s*\(", src, flags=re.M), name
    assert re.search(r"^#define\s+SPL_ABI_VERSION\s+11\s*$", src, flags=re.M)     # additive: no bump


@needs_lib
@pytest.mark.parametrize("n", (2, 3, 4))
def test_stage_bytes_match_documented_layout(n):
    from splendor import _lib
    L = _lib.lib()
    assert {2: 60, 3: 76, 4: 92}[n] * 7 * 32 == documented_bytes(n, 32) - documented_bytes(n, 0) - 128 - 1792
    for B in (0, 1, 31, 32, 33, 63, 64, 65, 200, 4096, 32768, 64 * 513 + 5):
        assert L.spl_nn_stage_bytes(n, B) == documented_bytes(n, B), B
        assert L.spl_nn_stage_bytes(n, B) % 16 == 0


@needs_lib
def test_stage_bytes_rejects_bad_arguments():
    from splendor import _lib
    L = _lib.lib()
    assert L.spl_abi_version() == 11 and _lib.ABI_VERSION == 11
    for n, B in ((1, 64), (5, 64), (2, -1)):
        assert L.spl_nn_stage_bytes(n, B) == _lib.EINVAL


@needs_lib
def test_staged_entry_points_reject_bad_arguments():
    """NULL or misaligned pointers and a precision outside 0 .. 2 are SPL_EINVAL before any
    launch (the calls below would otherwise launch on host memory)."""
    from splendor import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p, odd = vp(base), vp(base + 8)                     # 64-byte aligned / 8 but not 16

    def fwd(n=2, B=64, stage=p, w=p, pi=p, v=p, precision=0):
        return L.spl_nn_forward_staged(n, B, stage, w, pi, v, precision, None)
    for bad in (dict(n=1), dict(n=5), dict(B=-1), dict(stage=None), dict(w=None), dict(pi=None), dict(v=None),
                dict(stage=odd), dict(w=odd), dict(precision=-1), dict(precision=3)):
        assert fwd(**bad) == _lib.EINVAL, bad
    assert fwd(B=0) == 0                                # nothing to launch

    h = vp()
    assert L.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    try:
        def stg(ctx=h, B=64, state=p, valid=p, mask=p, stage=p):
            return L.spl_nn_stage_leaves(ctx, B, state, valid, mask, stage, None)
        for bad in (dict(ctx=None), dict(B=-1), dict(state=None), dict(valid=None), dict(mask=None),
                    dict(stage=None), dict(valid=odd), dict(stage=odd), dict(mask=vp(base + 4)),
                    dict(state=vp(base + 2))):
            assert stg(**bad) == _lib.EINVAL, bad
        assert stg(B=0) == 0
    finally:
        L.spl_ctx_destroy(h)
    for bad in ((None, p, p, p, p), (p, None, p, p, p)):   # no handle (checked first), no boards
        assert L.spl_mcts_select_staged(bad[0], bad[1], bad[2], bad[3], bad[4], None) == _lib.EINVAL
    assert {"spl_nn_stage_bytes", "spl_nn_stage_leaves", "spl_nn_forward_staged",
            "spl_mcts_select_staged"} <= set(_lib.exported_symbols())
