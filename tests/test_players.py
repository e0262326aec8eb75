"""The rule-based players, host side: the argument checks of spl_player_move (no device is
touched: every call returns before a launch), the integrity of the players fixtures
(tests/golden/players_*p.npz, the reference's legality and one-move scores on canonical
positions), the CPU oracle's rules against them, and the restated greedy rule."""
import ctypes
import os

import numpy as np
import pytest

import _oracle as O
import _players as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")


def test_entry_point_checks_arguments():
    """spl_player_move: SPL_EINVAL for a NULL ctx / state / action, B < 0, a kind outside
    0..2, POLICY without pi, a stream above 0xFFFFFF; 0 without a launch for B == 0; the
    symbol is exported and the ABI version unchanged."""
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.spl_abi_version() == 11
    move = lib.spl_player_move
    move.argtypes = [vp, ci, vp, vp, ci, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    move.restype = ci
    h = vp()
    lib.spl_ctx_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    assert lib.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    p = vp(16)                                   # never dereferenced: every call returns before a launch

    def call(ctx=h, B=4, state=p, active=None, kind=0, pi=None, stream=0, action=p):
        return move(ctx, B, state, active, kind, pi, 5, stream, 0, action, None, None, None)
    assert call(ctx=None) == -1
    assert call(state=None) == -1
    assert call(action=None) == -1
    assert call(B=-1) == -1
    assert call(kind=-1) == -1 and call(kind=3) == -1
    assert call(kind=2, pi=None) == -1
    assert call(stream=0x1000000) == -1
    for kind in (0, 1, 2):                       # the same checks come before the B == 0 return
        assert call(B=0, kind=kind, pi=p) == 0
        assert call(B=0, kind=kind, pi=p, stream=0xFFFFFF, active=p) == 0
        assert call(B=0, kind=kind, pi=p, state=None) == -1
        assert call(B=0, kind=kind, pi=p, stream=0x1000000) == -1
    assert call(B=0, kind=2, pi=None) == -1
    lib.spl_ctx_destroy.argtypes = [vp]
    lib.spl_ctx_destroy(h)
    from splendor import _lib
    assert "spl_player_move" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 11
    assert (_lib.PLAYER_RANDOM, _lib.PLAYER_GREEDY, _lib.PLAYER_POLICY) == (0, 1, 2)


@pytest.mark.parametrize("n", (2, 3, 4))
def test_fixture_classes(n):
    """At most 256 canonical positions, each class of the greedy rule at least 8 times, the
    stored class bits what the stored arrays say."""
    d = P.fixture(n)
    count = len(d["board"])
    assert 5 * P.CLASS_MIN <= count <= 256
    assert d["board"].shape == (count, O.rows(n), 7) and d["board"].dtype == np.int8
    assert d["valid"].shape == d["after"].shape == (count, 409)
    assert os.path.getsize(os.path.join(P.GOLD, f"players_{n}p.npz")) < 200 * 1024
    cls = np.zeros(count, np.uint8)
    for i in range(count):
        v, s0, after = d["valid"][i].astype(bool), int(d["s0"][i]), d["after"][i]
        assert v.any() and (after[~v] == -1).all() and (after[v] >= s0).all()
        m = int(after[v].max())
        scoring = after[v & (after > s0)]
        if m > s0:
            cls[i] = (1 if len(np.unique(scoring)) >= 2 else 0) | (2 if int((after[v] == m).sum()) >= 2 else 0)
        else:
            cls[i] = 4 if v[:12].any() else (8 if v[30:60].any() else 16)
    np.testing.assert_array_equal(cls, d["cls"])
    for k in range(5):
        assert int(((cls >> k) & 1).sum()) >= P.CLASS_MIN, f"class {k}"


@pytest.mark.parametrize("n", (2, 3, 4))
def test_oracle_reproduces_fixture(n):
    """The CPU oracle's valid_moves / make_move / get_score give the reference's legality,
    score and every one-move score on exactly these boards."""
    d = P.fixture(n)
    for i, board in enumerate(d["board"]):
        valid = O.valid_moves(n, board, 0)
        np.testing.assert_array_equal(valid, d["valid"][i], err_msg=f"position {i}")
        assert O.score(n, board, 0) == d["s0"][i], f"position {i}"
        np.testing.assert_array_equal(P.oracle_after(O, n, board, valid), d["after"][i], err_msg=f"position {i}")


def test_restated_greedy_rule():
    """The numpy restatement on hand-made cases, one per branch."""
    valid = np.zeros(409, bool)
    after = np.full(409, -1)
    legal = [3, 7, 28, 31, 40, 100]
    valid[legal] = True
    after[legal] = 2
    c, m = P.greedy_candidates(valid, 2, after)              # nothing scores: visible buys
    assert m == 2 and np.flatnonzero(c).tolist() == [3, 7]
    after[[7, 28]] = 5
    after[3] = 4
    c, m = P.greedy_candidates(valid, 2, after)              # the tie for the best gain
    assert m == 5 and np.flatnonzero(c).tolist() == [7, 28]
    valid[[3, 7]] = False
    after[[3, 7]] = -1
    after[28] = 2
    c, m = P.greedy_candidates(valid, 2, after)              # a reserved buy is no visible buy: gems
    assert m == 2 and np.flatnonzero(c).tolist() == [31, 40]
    valid[[31, 40]] = False
    after[[31, 40]] = -1
    c, m = P.greedy_candidates(valid, 2, after)              # neither: every legal move
    assert np.flatnonzero(c).tolist() == [28, 100]
    assert P.pick(c, 0.0) == 28 and P.pick(c, 0.4999) == 28 and P.pick(c, 0.5) == 100
    pi = np.zeros(409, np.float32)
    pi[[28, 100]] = 0.25
    pi[5] = 0.9                                              # illegal
    assert np.flatnonzero(P.policy_candidates(valid, pi)).tolist() == [28, 100]
