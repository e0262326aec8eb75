"""The rules word of the context (spl_ctx_set_rules / spl_ctx_rules, no GPU needed) and the
rule the GPU tests use: on every position of the reserve-free fixtures (the reference run with
ENABLE_ACTION_RESERVE = False, make_rules_golden.py) the recorded mask equals
_rules.no_reserve(the full game's mask from the CPU oracle)."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import _rules as R


def test_rules_word_round_trip():
    from splendor import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    try:
        assert L.spl_ctx_rules(h) == 0                           # the full game by default
        assert L.spl_ctx_set_rules(h, _lib.RULE_NO_RESERVE) == 0
        assert L.spl_ctx_rules(h) == _lib.RULE_NO_RESERVE == R.RULE_NO_RESERVE
        for bad in (2, 3, 0x100, -1, 1 << 30):                   # unknown bits: refused, nothing changed
            assert L.spl_ctx_set_rules(h, bad) == _lib.EINVAL
            assert L.spl_ctx_rules(h) == _lib.RULE_NO_RESERVE
        assert L.spl_ctx_set_token_limit(h, 9) == 0              # the limit and the flags are independent
        assert L.spl_ctx_rules(h) == _lib.RULE_NO_RESERVE
        assert L.spl_ctx_set_rules(h, 0) == 0
        assert L.spl_ctx_rules(h) == 0
    finally:
        L.spl_ctx_destroy(h)
    assert L.spl_ctx_set_rules(None, 0) == _lib.EINVAL
    assert L.spl_ctx_rules(None) == _lib.EINVAL
    assert L.spl_mcts_rules(None) == _lib.EINVAL
    assert L.spl_abi_version() == 11


@pytest.mark.parametrize("n", (2, 3, 4))
def test_env_fixture_masks_are_the_rule(n):
    d = R.fixture(f"noreserve_env_{n}p.npz")
    canon = np.stack([O.valid_moves(n, s, 0) for s in d["canon"]])
    mover = np.stack([O.valid_moves(n, s, int(p)) for s, p in zip(d["state"], d["player"])])
    np.testing.assert_array_equal(d["mask_canon"].astype(bool), R.no_reserve(canon))
    np.testing.assert_array_equal(d["mask_player"].astype(bool), R.no_reserve(mover))
    # what the rule changes and what it leaves alone, both present
    assert canon[:, R.RSV].any() and not d["mask_canon"][:, R.RSV].any()
    assert d["mask_canon"][:, R.RSV_GIVE].any()
    np.testing.assert_array_equal(d["mask_canon"][:, R.RSV_GIVE], canon[:, R.RSV_GIVE])
    assert d["mask_player"][np.arange(len(d["action"])), d["action"]].all()
    assert not np.isin(d["action"], np.arange(12, 27)).any()


def test_env_fixtures_hold_a_pass_made_by_the_rule():
    """A position whose only legal moves were reserves passes under the rule."""
    made = 0
    for n in (3, 4):
        d = R.fixture(f"noreserve_env_{n}p.npz")
        for s in d["canon"][d["mask_canon"][:, R.PASS] != 0]:
            made += not O.valid_moves(n, s, 0)[R.PASS]
    assert made >= 1


@pytest.mark.parametrize("n", (2, 4))
def test_search_fixture_roots_follow_the_rule(n):
    d = R.fixture(f"noreserve_mcts_{n}p.npz")
    for roots, counts in ((d["root"], d["counts"]), (d["seq_root"], d["seq_counts"])):
        legal = R.no_reserve(np.stack([O.valid_moves(n, s, 0) for s in roots]))
        assert not counts[~legal].any()
        assert not counts[:, R.RSV].any() and counts[:, R.RSV_GIVE].any()
    assert len(d["root"]) == 18 and len(d["seq_root"]) == 30


@pytest.mark.parametrize("tag,n", (("2p", 2), ("4p", 4)))
def test_episode_fixture_valids_are_the_rule(tag, n):
    d = R.fixture(f"noreserve_episode_{tag}.npz")
    legal = R.no_reserve(np.stack([O.valid_moves(n, s, 0) for s in d["board"]]))
    np.testing.assert_array_equal(d["valids"].astype(bool), legal)
    assert not d["pi"][~legal].any()
    acts = d["game_actions"][d["game_actions"] >= 0]
    assert not np.isin(acts, np.arange(12, 27)).any()
    if n == 4:
        assert np.isin(acts, np.arange(290, 365)).any() and (acts == R.PASS).any()
