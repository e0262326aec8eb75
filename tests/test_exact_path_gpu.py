"""The exact-predicate path (boards with a negative byte) through k_playout and k_leaf_mask. All
three lane-per-board kernels build their masks with the same two phases (csrc/board_phases.h);
test_rules_gpu.py::test_masks_on_arbitrary_byte_boards pins the path for spl_valid_moves and
k_rollout, this file for the other two callers, on the first 96 of that test's boards (one full
64-board workgroup and a partial one), under the full rules and the reserve-free ones."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _oracle as O  # noqa: E402
import _players as P  # noqa: E402
import _rules as R  # noqa: E402

pytestmark = pytest.mark.gpu

B = 96
SENTINEL = -5
CASES = [(n, rule) for n in (2, 3, 4) for rule in (False, True)]


@functools.lru_cache(maxsize=None)
def boards(n):
    """test_masks_on_arbitrary_byte_boards' construction (same fixture, seed and draws; the draws
    of board b follow those of boards 0 .. b - 1 only), with the oracle's full-rules masks for
    player 0 (the leaf masks' player) and for the row's own player. Read-only, shared."""
    d = R.fixture(f"noreserve_env_{n}p.npz")
    rng = np.random.default_rng(31 + n)
    rows = O.rows(n)
    st, pl = d["state"][:B].copy(), d["player"][:B].astype(np.int8)
    hit = np.array([0] + list(range(1, 31)) + list(range(32 + n, rows)))
    for b in range(B):
        for _ in range(rng.integers(1, 6)):
            st[b, rng.choice(hit), rng.integers(0, 7)] = rng.integers(-128 if b % 2 else 0, 12)
    seat0 = np.stack([O.valid_moves(n, st[b], 0) for b in range(B)])
    mover = np.stack([O.valid_moves(n, st[b], int(pl[b])) for b in range(B)])
    for a in (st, pl, seat0, mover):
        a.setflags(write=False)
    return st, pl, seat0, mover


def on_exact_path(n, st, player):
    """Boards with a negative colour byte in a row the predicates of `player` read (bank, the
    player's gems, cards and reserve, the visible cards' costs, the deck counts): the boards the
    kernels send down the exact path. The fixture's own boards have none there."""
    gems, cards, rsv = 32 + n, 32 + 3 * n + n * n, 32 + 4 * n + n * n
    out = np.zeros(len(st), bool)
    for b, p in enumerate(np.broadcast_to(player, len(st))):
        rows = [0, gems + p, cards + p, rsv + 6 * p + 5] + [1 + 2 * i for i in range(12)] + \
               [25 + 2 * t for t in range(3)] + [rsv + 6 * p + 2 * t for t in range(3)]
        out[b] = (st[b, rows, :5] < 0).any()
    return out


def guard(n, st, player):
    """At least a quarter of the boards carry a negative byte (the construction gives half; the
    fixture's own boards carry some too, outside the rows the predicates read), and the exact path
    itself is taken in both workgroups: by at least 1 board in 16 of each. An odd board gets 1-5
    overwrites, 128 in 140 of them negative, about 1 in 4 of them on a colour byte of a row its
    player's predicates read, so about 2 boards in 9 are expected there; 1 in 16 leaves room for
    the draw and still puts several boards of either workgroup on the path."""
    assert (st < 0).any(axis=(1, 2)).sum() >= B // 4
    exact = on_exact_path(n, st, player)
    assert exact[:64].sum() >= 4 and exact[64:].sum() >= 2


def want_mask(oracle, rule):
    return R.no_reserve(oracle) if rule else oracle.astype(bool)


def engine(n, rule):
    from splendor.env import SplendorEngine
    e = SplendorEngine(n, device="cuda")
    e.set_rules(no_reserve=rule)
    return e


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


@pytest.mark.parametrize("pattern", ("all", "random"))
@pytest.mark.parametrize("n,rule", CASES)
def test_leaf_masks(n, rule, pattern):
    """spl_nn_stage_leaves (k_leaf_mask, staged): masks by tree row, the staged masks in list
    order, the sentinel on unlisted rows."""
    from splendor import _lib
    from splendor.env import _ptr
    from splendor.nnet import new_stage
    st, _, seat0, _ = boards(n)
    guard(n, st, 0)
    want = want_mask(seat0, rule)
    valid = np.ones(B, np.uint8)
    if pattern == "random":
        valid[:] = np.random.default_rng(900 + n).random(B) < 0.7
    listed = np.nonzero(valid)[0]
    e = engine(n, rule)
    by_tree = torch.full((B, 7), SENTINEL, dtype=torch.int64, device="cuda")
    stage = new_stage(n, B, "cuda")
    dst, dvalid = dev(st), dev(valid)                            # (named: alive until the results are read)
    _lib.check(e.L.spl_nn_stage_leaves(e.ctx, B, _ptr(dst), _ptr(dvalid), _ptr(by_tree), _ptr(stage), e._s()),
               "spl_nn_stage_leaves")
    got = by_tree.cpu().numpy()
    np.testing.assert_array_equal(P.unpack(got[listed]), want[listed])
    assert (got[valid == 0] == SENTINEL).all()
    total = int(stage[:4].view(torch.int32).item())
    assert total == len(listed)
    m_off = (16 + 4 * B + 15) // 16 * 16
    np.testing.assert_array_equal(stage[16:16 + 4 * total].view(torch.int32).cpu().numpy(), listed)
    staged = stage[m_off:m_off + 56 * total].view(torch.int64).view(-1, 7).cpu().numpy()
    np.testing.assert_array_equal(P.unpack(staged), want[listed])


@pytest.mark.parametrize("n,rule", CASES)
def test_playout_prior(n, rule):
    """spl_playout, one playout of one move with pi_out (k_playout's first mask): each row's prior
    is 1 / count on exactly the legal moves of the row's player."""
    st, pl, _, mover = boards(n)
    guard(n, st, pl)
    want = want_mask(mover, rule)
    count = want.sum(1)
    assert (count > 0).all()                                     # (the pass bit when nothing else is legal)
    e = engine(n, rule)
    out = e.playout(dev(st), dev(pl), policy="uniform", playouts=1, max_steps=1, seed=0x5EED, pi=True)
    pi = out["pi"].cpu().numpy()
    np.testing.assert_array_equal(pi != 0, want)
    np.testing.assert_array_equal(pi, np.where(want, (np.float32(1.0) / count.astype(np.float32))[:, None],
                                               np.float32(0)))
