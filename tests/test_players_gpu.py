"""spl_player_move on the device against the players fixtures (the reference's legality and
one-move scores, tests/golden/players_*p.npz) and the numpy restatement of the candidate
rules (_players.py): candidate sets, best scores and the keyed choice, bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _oracle as O  # noqa: E402
import _players as P  # noqa: E402

pytestmark = pytest.mark.gpu

RANDOM, GREEDY, POLICY = 0, 1, 2


def engine(n):
    from splendor.env import SplendorEngine
    return SplendorEngine(n, device="cuda")


def run(e, boards, kind, active=None, pi=None, seed=0, stream=0, board_base=0, sentinel=-7):
    """-> (action, cand bool [B,409], best), as numpy; outputs pre-filled with `sentinel`."""
    B, dev = len(boards), e.device
    st = torch.from_numpy(np.array(boards, np.int8)).to(dev)      # (a writable copy)
    fill = sentinel
    action = torch.full((B,), fill, dtype=torch.int16, device=dev)
    cand = torch.full((B, 7), fill, dtype=torch.int64, device=dev)
    best = torch.full((B,), fill, dtype=torch.int32, device=dev)
    e.player_move(st, kind, active=None if active is None else torch.from_numpy(active).to(dev),
                  pi=None if pi is None else torch.from_numpy(np.array(pi, np.float32)).to(dev), seed=seed, stream=stream,
                  board_base=board_base, out=action, cand_out=cand, best_out=best)
    torch.cuda.synchronize()
    return action.cpu().numpy(), cand.cpu().numpy(), best.cpu().numpy()


def expected(d):
    """Per position: (greedy candidate mask, m) from the fixture's arrays."""
    c, m = zip(*(P.greedy_candidates(d["valid"][i], int(d["s0"][i]), d["after"][i]) for i in range(len(d["s0"]))))
    return np.array(c), np.array(m)


def check_choice(action, cand, seed, stream, board_base, rows=None):
    for b in (range(len(action)) if rows is None else rows):
        u = O.uniform(seed, board_base + b, P.ST_PLAYER | stream, 0)
        assert action[b] == P.pick(cand[b], u), f"board {b}"


@pytest.mark.parametrize("n", (2, 3, 4))
def test_player_move_matches_reference(n):
    d = P.fixture(n)
    e = engine(n)
    gc, gm = expected(d)
    for seed, stream, base in ((0x5EED, 0, 0), (0xABCDEF0123456789, 0xFFFFFF, 0xFFFFFF00)):
        a, c, best = run(e, d["board"], GREEDY, seed=seed, stream=stream, board_base=base)
        np.testing.assert_array_equal(P.unpack(c), gc)
        np.testing.assert_array_equal(best, gm)
        check_choice(a, gc, seed, stream, base)
        a, c, best = run(e, d["board"], RANDOM, seed=seed, stream=stream, board_base=base)
        np.testing.assert_array_equal(P.unpack(c), d["valid"].astype(bool))
        np.testing.assert_array_equal(best, d["s0"])
        check_choice(a, d["valid"], seed, stream, base)


@pytest.mark.parametrize("kind", (RANDOM, GREEDY, POLICY))
def test_inactive_rows_keep_sentinels(kind):
    n = 2
    d = P.fixture(n)
    e = engine(n)
    B = 67
    boards = d["board"][:B]
    active = (np.arange(B) % 3 != 1).astype(np.uint8)
    pi = np.random.default_rng(3).random((B, 409)).astype(np.float32)
    a, c, best = run(e, boards, kind, active=active, pi=pi if kind == POLICY else None, seed=9, stream=4,
                     board_base=100, sentinel=-7)
    off = active == 0
    assert (a[off] == -7).all() and (c[off] == -7).all() and (best[off] == -7).all()
    on = np.flatnonzero(active)
    want = {RANDOM: d["valid"][:B].astype(bool), GREEDY: expected(d)[0][:B],
            POLICY: np.array([P.policy_candidates(d["valid"][i], pi[i]) for i in range(B)])}[kind]
    np.testing.assert_array_equal(P.unpack(c)[on], want[on])
    check_choice(a, want, 9, 4, 100, rows=on)


@pytest.mark.parametrize("B", (1, 5, 67))
def test_batch_sizes(B):
    """One board, a partial workgroup, and a batch that ends inside a workgroup."""
    n = 3
    d = P.fixture(n)
    e = engine(n)
    gc, gm = expected(d)
    rows = np.arange(B) * 3 % len(d["board"])                # positions of every class
    a, c, best = run(e, d["board"][rows], GREEDY, seed=11, stream=B, board_base=7)
    np.testing.assert_array_equal(P.unpack(c), gc[rows])
    np.testing.assert_array_equal(best, gm[rows])
    check_choice(a, gc[rows], 11, B, 7)


@pytest.mark.parametrize("n", (2, 4))
def test_policy_player(n):
    """Crafted priors on fixture boards: exact ties among legal moves, strictly larger
    values on illegal moves, a legal maximum of 0.0, and plain random priors."""
    d = P.fixture(n)
    e = engine(n)
    B = 64
    boards, valid = d["board"][:B], d["valid"][:B].astype(bool)
    rng = np.random.default_rng(40 + n)
    pi = rng.random((B, 409)).astype(np.float32)
    for b in range(B):
        legal, illegal = np.flatnonzero(valid[b]), np.flatnonzero(~valid[b])
        mode = b % 4
        if mode == 0:                                        # a tie among (up to) three legal moves
            pi[b, legal[rng.permutation(len(legal))[:3]]] = np.float32(1.5)
        elif mode == 1:                                      # illegal moves above every legal one
            pi[b, illegal] = np.float32(2.0) + rng.random(len(illegal)).astype(np.float32)
        elif mode == 2:                                      # legal maximum 0.0 (all legal entries zero)
            pi[b, legal] = 0.0
            pi[b, illegal[::2]] = -1.0
    want = np.array([P.policy_candidates(valid[b], pi[b]) for b in range(B)])
    assert (want.sum(1)[0::4] == np.minimum(3, valid.sum(1))[0::4]).all()
    assert (want[2::4] == valid[2::4]).all()
    a, c, best = run(e, boards, POLICY, pi=pi, seed=77, stream=12, board_base=3)
    np.testing.assert_array_equal(P.unpack(c), want)
    np.testing.assert_array_equal(best, d["s0"][:B])
    check_choice(a, want, 77, 12, 3)


def test_token_limit_is_the_contexts():
    n = 2
    d = P.fixture(n)
    e = engine(n)
    st = torch.from_numpy(np.array(d["board"], np.int8)).to(e.device)
    e.set_token_limit(9)
    lim9 = e.valid_moves(st).cpu().numpy()
    _, c, _ = run(e, d["board"], RANDOM, seed=1)
    np.testing.assert_array_equal(c, lim9)
    assert (P.unpack(lim9) != d["valid"].astype(bool)).any()     # (the limit changes some masks)
    e.set_token_limit(10)
    _, c, _ = run(e, d["board"], RANDOM, seed=1)
    np.testing.assert_array_equal(P.unpack(c), d["valid"].astype(bool))
