"""BatchedPit (pit.py with the players of SplendorPlayers.py, batched) against a sequential
restatement on the oracle, written like test_arena_gpu.oracle_arena: per game the seats of
Arena.py:200-203, per ply the mover's rule (search with the Philox tie-break, the greedy /
random / arg-max-policy candidate sets of _players.py with the keyed choice), chance steps
on the game's Philox stream. Move for move: actions, plies, results, final scores, totals."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _oracle as O  # noqa: E402
import _players as P  # noqa: E402

pytestmark = pytest.mark.gpu

ST_BEST = 6 << 24
DEAL_DRAWS = 29
MEM = 1 << 28            # bytes for a pit's trees: a few small games (the default plans most of the free HBM)


def oracle_move(n, spec, tree, canon, seed, board, ply):
    valid = O.valid_moves(n, canon, 0)
    if spec[0] == "mcts":
        counts = tree.search(canon)[0]
        u = O.uniform(seed, board, ST_BEST | ply, 0)
        top = counts.max()
        if top == 0:
            return int(u * 409)
        best = np.flatnonzero(counts == top)
        return int(best[int(u * len(best))])
    if spec[0] == "greedy":
        cand = P.greedy_candidates(valid, O.score(n, canon, 0), P.oracle_after(O, n, canon, valid))[0]
    elif spec[0] == "policy":
        cand = P.policy_candidates(valid, O.fake_predict(n, canon, valid)[0])
    else:
        cand = valid.astype(bool)
    return P.pick(cand, O.uniform(seed, board, P.ST_PLAYER | ply, 0))


def oracle_pit(n, G, specs, seed, game_base=0):
    """specs: two of ("mcts", sims, cpuct, fpu) / ("greedy",) / ("random",) / ("policy",)."""
    from splendor.arena import one_vs_two
    out = []
    for gid in range(G):
        board = game_base + gid
        st, _ = O.init(n, [O.uniform(seed, board, 0xFFFFFFFF, k) for k in range(DEAL_DRAWS)])
        seats = [0] + [1] * (n - 1) if one_vs_two(gid) else [1] + [0] * (n - 1)
        trees = [O.Mcts(n, s[1], s[2], s[3], False) if s[0] == "mcts" else None for s in specs]
        result, plies, actions = np.zeros(n, np.float32), 0, []
        for ply in range(62 * n * 2 + 8):
            cur = ply % n
            canon = O.swap_players(n, st, cur) if cur else st.copy()
            k = seats[cur]
            a = oracle_move(n, specs[k], trees[k], canon, seed ^ (k + 1), board, ply)
            assert O.valid_moves(n, canon, 0)[a]
            actions.append(a)
            st, _, _ = O.make_move(n, st, a, cur, False, [O.uniform(seed, board, ply, d) for d in range(8)])
            r = O.check_end(n, st)
            if r.any():
                result, plies = r, ply + 1
                break
        out.append((result, plies, [O.score(n, st, p) for p in range(n)], actions))
    return out


def seat(spec, engine):
    from splendor import pit
    from splendor.mcts import HashEvaluator
    if spec[0] == "mcts":
        return pit.MCTSPlayer(None, numMCTSSims=spec[1], cpuct=spec[2], fpu=spec[3], evaluator=HashEvaluator(engine))
    if spec[0] == "policy":
        return pit.PolicyPlayer(None, evaluator=HashEvaluator(engine))
    return pit.GreedyPlayer() if spec[0] == "greedy" else pit.RandomPlayer()


GREEDY, RANDOM, POLICY = ("greedy",), ("random",), ("policy",)
CASES = [(2, 12, GREEDY, RANDOM), (3, 6, GREEDY, RANDOM),
         (2, 8, ("mcts", 6, 1.5, 0.1), GREEDY),
         (2, 8, ("mcts", 4, 1.5, 0.1), ("mcts", 8, 1.0, 0.0)),
         (2, 8, POLICY, RANDOM)]


@pytest.mark.parametrize("n,G,one,two", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pit_matches_oracle(n, G, one, two):
    from splendor.SplendorGame import SplendorGame
    from splendor.arena import one_vs_two
    from splendor.pit import BatchedPit
    seed, base = 33, 5
    g = SplendorGame(n)
    # (args' search settings differ from every player's own: a player's own must win)
    pit = BatchedPit(g, seat(one, g.engine), seat(two, g.engine), dict(numMCTSSims=3, cpuct=9.0, fpu=0.7),
                     batch=G, seed=seed, game_base=base, mem_budget=MEM)
    won1, won2, draws = pit.playGames(G)
    ref = oracle_pit(n, G, (one, two), seed, base)
    last = pit.last
    for i, (r, plies, score, actions) in enumerate(ref):
        assert last["plies"][i] == plies, f"game {i}"
        np.testing.assert_array_equal(last["actions"][i][:plies], actions, err_msg=f"game {i}")
        assert (last["actions"][i][plies:] == -1).all()
        np.testing.assert_array_equal(last["result"][i], r, err_msg=f"game {i}")
        np.testing.assert_array_equal(last["score"][i], score)
    r0 = np.array([r[0][0] for r in ref])
    ovt = np.array([one_vs_two(i) for i in range(G)])
    np.testing.assert_array_equal(last["one_vs_two"], ovt)
    np.testing.assert_array_equal(last["game"], np.arange(G))
    assert won1 == int(np.sum(np.where(ovt, r0 == 1.0, r0 == -1.0)))
    assert won2 == int(np.sum(np.where(ovt, r0 == -1.0, r0 == 1.0)))
    assert won1 + won2 + draws == G
    assert pit.capacity == {"prunes": 0, "resets": 0, "unexpanded": 0}


class NegatedHash:
    """The arena fixture's second network: the hash network with values negated."""

    def __init__(self, engine):
        from splendor.mcts import HashEvaluator
        self.h = HashEvaluator(engine)

    def __call__(self, leaf_state, leaf_mask, leaf_valid):
        pi, v = self.h(leaf_state, leaf_mask, leaf_valid)
        return pi, -v


def test_equal_search_players_are_the_arena():
    """Two MCTSPlayers with the arena's settings: every key of .last equals
    BatchedArena.last for the same seed."""
    from splendor.SplendorGame import SplendorGame
    from splendor.arena import BatchedArena
    from splendor.mcts import HashEvaluator
    from splendor.pit import BatchedPit, MCTSPlayer
    g = SplendorGame(2)
    args = dict(numMCTSSims=5, cpuct=1.5, fpu=0.1)
    ev = (HashEvaluator(g.engine), NegatedHash(g.engine))
    ar = BatchedArena(g, None, None, args, batch=8, seed=17, game_base=3, evaluators=ev,
                      mem_budget=MEM)
    want = ar.playGames(8)
    pit = BatchedPit(g, MCTSPlayer(None, evaluator=ev[0]), MCTSPlayer(None, evaluator=ev[1]), args, batch=8,
                     seed=17, game_base=3, mem_budget=MEM)
    assert pit.playGames(8) == want
    assert set(pit.last) == set(ar.last) == {"game", "one_vs_two", "result", "plies", "score", "actions"}
    for k in ar.last:
        np.testing.assert_array_equal(pit.last[k], ar.last[k], err_msg=k)


def test_pit_matches_reference_arena():
    """tests/golden/arena_2p.npz (the reference's Arena.playGames with two MCTS players)
    through BatchedPit: every move, per-game results, totals."""
    from splendor.SplendorGame import SplendorGame
    from splendor.mcts import HashEvaluator
    from splendor.pit import BatchedPit, MCTSPlayer
    with np.load(os.path.join(P.GOLD, "arena_2p.npz")) as z:
        d = {k: z[k] for k in z.files}
    G = len(d["plies"])
    g = SplendorGame(2)
    kw = dict(numMCTSSims=int(d["sims"]), cpuct=float(d["cpuct"]), fpu=float(d["fpu"]))
    pit = BatchedPit(g, MCTSPlayer(None, evaluator=HashEvaluator(g.engine), **kw),
                     MCTSPlayer(None, evaluator=NegatedHash(g.engine), **kw), batch=G, seed=int(d["seed"]),
                     mem_budget=MEM)
    totals = pit.playGames(G)
    last = pit.last
    for i in range(G):
        p = int(d["plies"][i])
        assert last["plies"][i] == p, f"game {i}"
        np.testing.assert_array_equal(last["actions"][i][:p], d["actions"][i][:p], err_msg=f"game {i}")
        assert [float(last["result"][i][0]), float(last["score"][i][0]), float(last["score"][i][1])] == \
            list(d["result"][i])
    assert totals == (int(d["one"]), int(d["two"]), int(d["draws"]))


def test_pit_batches():
    """Games split over several batches give the same per-game records as one batch."""
    from splendor.SplendorGame import SplendorGame
    from splendor.mcts import HashEvaluator
    from splendor.pit import BatchedPit, GreedyPlayer, MCTSPlayer
    g = SplendorGame(2)
    last = []
    for batch in (8, 3):
        pit = BatchedPit(g, MCTSPlayer(None, numMCTSSims=4, evaluator=HashEvaluator(g.engine)), GreedyPlayer(),
                         batch=batch, seed=5, mem_budget=MEM)
        pit.playGames(8)
        last.append(pit.last)
    for k in ("game", "one_vs_two", "result", "plies", "score", "actions"):
        np.testing.assert_array_equal(last[0][k], last[1][k], err_msg=k)


def test_treeless_pairing_allocates_no_tree(monkeypatch):
    from splendor import arena, pit
    from splendor.SplendorGame import SplendorGame

    def no_tree(*a, **k):
        raise AssertionError("a BatchedMCTS was created for a tree-less pairing")
    monkeypatch.setattr(pit, "BatchedMCTS", no_tree)
    monkeypatch.setattr(arena, "BatchedMCTS", no_tree)
    g = SplendorGame(2)
    p = pit.BatchedPit(g, pit.GreedyPlayer(), pit.RandomPlayer(), batch=4, seed=2)
    assert p.mcts == []
    assert sum(p.playGames(4)) == 4
    assert p.capacity == {"prunes": 0, "resets": 0, "unexpanded": 0}
    with pytest.raises(TypeError):
        pit.BatchedPit(g, pit.GreedyPlayer(), "random", batch=4)


def test_sequential_players():
    """SplendorPlayers' one-board form: the reference's Arena over the Game API finishes,
    and GreedyPlayer.play returns a member of the restated candidate set."""
    from splendor.SplendorGame import SplendorGame
    from splendor.SplendorPlayers import GreedyPlayer, RandomPlayer
    from splendor.arena import Arena
    g = SplendorGame(2)
    greedy, rand = GreedyPlayer(g), RandomPlayer(g)
    one, two, draws = Arena(greedy.play, rand.play, None, g).playGames(2)
    assert one + two + draws == 2
    d = P.fixture(2)
    for i in np.flatnonzero(d["cls"] & 3)[:4].tolist() + np.flatnonzero(d["cls"] & 28)[::40][:4].tolist():
        cand, _ = P.greedy_candidates(d["valid"][i], int(d["s0"][i]), d["after"][i])
        assert cand[greedy.play(np.array(d["board"][i]))], f"position {i}"
        assert d["valid"][i][rand.play(np.array(d["board"][i]))], f"position {i}"
        assert d["valid"][i][rand.play(np.array(d["board"][i]), player=0)]
