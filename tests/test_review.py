"""CPU checks of the search review: the principal-variation entry is declared, exported and
bound (the ABI version stays 11), rejects a NULL handle before any launch, and the numpy
post-processing of splendor.review (rank_moves, entropy, summarise) on hand-made arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splendor_amd.h")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")

DEFINES = {"SPL_PV_MAX_LINES": 16, "SPL_PV_MAX_DEPTH": 64, "SPL_PV_END_DEPTH": 0, "SPL_PV_END_UNLINKED": 1,
           "SPL_PV_END_TERMINAL": 2, "SPL_PV_END_UNVISITED": 3, "SPL_PV_END_NONE": 4, "SPL_ABI_VERSION": 11}


def pv_prototype():
    src = open(HEADER).read()
    m = re.search(r"^int\s+spl_mcts_pv\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "spl_mcts_pv is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_pv_and_defines():
    src = open(HEADER).read()
    for name, value in DEFINES.items():
        m = re.search(rf"^#define\s+{name}\s+(\S+)", src, flags=re.M)
        assert m and int(m.group(1)) == value, name
    assert pv_prototype() == ["spl_mcts *m", "int lines", "int depth", "int16_t *action", "int32_t *visits",
                              "double *q", "float *prior", "int32_t *length", "uint8_t *end", "void *hip_stream"]


def test_library_exports_pv():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "spl_mcts_pv")
    assert lib.spl_abi_version() == 11


def test_binding_lists_pv():
    """One ctypes argument per parameter of the header's prototype (handle, lines, depth, four
    entry arrays, length, end, stream), ints where the prototype has ints; the constants."""
    from splendor import _lib
    args, res = _lib._SIGS["spl_mcts_pv"]
    proto = pv_prototype()
    assert len(args) == len(proto) == 10
    assert [a is ctypes.c_int for a in args] == [p.startswith("int ") for p in proto]
    assert res is ctypes.c_int
    assert _lib.ABI_VERSION == 11
    assert (_lib.PV_MAX_LINES, _lib.PV_MAX_DEPTH) == (16, 64)
    assert (_lib.PV_END_DEPTH, _lib.PV_END_UNLINKED, _lib.PV_END_TERMINAL, _lib.PV_END_UNVISITED,
            _lib.PV_END_NONE) == (0, 1, 2, 3, 4)


def test_pv_rejects_a_null_handle():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.spl_mcts_pv.argtypes = [vp, ctypes.c_int, ctypes.c_int] + [vp] * 7
    dummy = vp(16)                                           # never dereferenced: rejected before any launch
    assert lib.spl_mcts_pv(None, 1, 1, dummy, None, None, None, dummy, None, None) == -1


# ------------------------------------------------------------------ numpy post-processing
def test_rank_moves_orders_by_visits_then_action():
    from splendor.review import rank_moves
    counts = np.zeros((3, 409), np.int64)
    counts[0, [5, 7, 300]] = [4, 9, 4]                       # a tie between 5 and 300
    counts[1, [408, 0]] = [2, 2]                             # a tie between the first and the last action
    order = rank_moves(counts)
    assert order.shape == (3, 409)
    assert order[0, :4].tolist() == [7, 5, 300, 0]           # ties go to the lower action; then the unvisited
    assert order[1, :3].tolist() == [0, 408, 1]
    assert order[2].tolist() == list(range(409))             # all-zero counts
    for r in order:
        assert sorted(r.tolist()) == list(range(409))
    assert rank_moves(counts[0]).tolist() == order[0].tolist()   # one row


def test_entropy():
    from splendor.review import entropy
    p = np.zeros((4, 409))
    p[0, 3] = 1.0
    p[1, [1, 2]] = 0.5
    p[2, :] = 1.0 / 409
    h = entropy(p)
    assert h[0] == 0.0 and h[3] == 0.0                       # one move; not searched (all zero)
    assert abs(h[1] - np.log(2.0)) < 1e-15
    assert abs(h[2] - np.log(409.0)) < 1e-12
    assert (h >= 0).all()


def test_summarise():
    from splendor.review import summarise
    N = 5
    counts = np.zeros((N, 409), np.int64)
    qsa = np.full((N, 409), -42.0)
    counts[0, [10, 20, 30]] = [6, 3, 1]; qsa[0, [10, 20, 30]] = [0.5, 0.25, -1.0]    # played the best
    counts[1, [10, 20, 30]] = [6, 3, 1]; qsa[1, [10, 20, 30]] = [0.5, 0.25, -1.0]    # played the third
    counts[2, [10, 20]] = [5, 5]; qsa[2, [10, 20]] = [0.1, 0.4]                      # a tie, played the higher action
    counts[3, [10, 20]] = [7, 3]; qsa[3, [10, 20]] = [0.2, 0.3]                      # played an unvisited move
    played = np.array([10, 30, 20, 50, 408])                                         # row 4: nothing searched
    probs = counts / np.maximum(counts.sum(1, keepdims=True), 1)
    value = np.array([0.5, 0.5, 0.25, 0.2, 0.0])
    s = summarise(counts, qsa, probs, value, played)
    assert s["best"].tolist() == [10, 10, 10, 10, 0]
    assert s["played"].tolist() == played.tolist()
    assert s["played_rank"].tolist() == [0, 2, 1, 50, 408]   # 50 follows 10, 20 and the 48 other actions below it
    assert s["visits"].tolist() == [10, 10, 10, 10, 0]
    assert s["best_visits"].tolist() == [6, 6, 5, 7, 0]
    assert s["played_visits"].tolist() == [6, 1, 5, 0, 0]
    np.testing.assert_allclose(s["best_share"], [0.6, 0.6, 0.5, 0.7, 0.0])
    np.testing.assert_allclose(s["played_share"], [0.6, 0.1, 0.5, 0.0, 0.0])
    np.testing.assert_array_equal(s["q_loss"][:3], [0.0, 1.5, 0.1 - 0.4])
    assert np.isnan(s["q_loss"][3]) and np.isnan(s["played_q"][3]) and s["best_q"][3] == 0.2
    assert np.isnan(s["q_loss"][4]) and np.isnan(s["best_q"][4]) and np.isnan(s["played_q"][4])
    np.testing.assert_array_equal(s["value"], value)
    np.testing.assert_allclose(s["entropy"][2], np.log(2.0))
    assert s["entropy"][4] == 0.0
    for k, v in s.items():
        assert v.shape == (N,), k
    empty = summarise(np.zeros((0, 409), np.int64), np.zeros((0, 409)), np.zeros((0, 409)), np.zeros(0),
                      np.zeros(0, np.int64))
    assert all(v.shape == (0,) for v in empty.values())
