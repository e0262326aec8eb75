"""spl_mcts_pv (BatchedMCTS.principal_variations) and splendor.review on the device.

The walk is checked against what the engine already reports: the root level against
root_stats / root_priors, the levels below it by re-rooting a handle at the line's child
(set_roots keeps the statistics) and reading root_stats there with no simulation in between.
Trees come from the hash network (no weights needed), games from the greedy / random players."""
import ctypes
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MEM = 1 << 28            # bytes for a handle's trees (the default plans most of the free HBM)
B = 6                    # trees: not a multiple of any workgroup's wave count
PASS = 408
FILL = dict(action=-1, visits=0, q=-42.0, prior=0.0)


@pytest.fixture(scope="module")
def engines():
    from splendor.env import SplendorEngine
    return {n: SplendorEngine(n) for n in (2, 3, 4)}


def midgame_roots(e, seed=11):
    """B canonical boards after 10 n random moves."""
    from splendor.env import RolloutBatch
    rb = RolloutBatch(e, B, seed=seed)
    for _ in range(10 * e.n):
        rb.step()
    assert int(rb.games.sum()) == 0
    return e.canonical(rb.state, rb.player)


def handle(e, sims, mode=0, batch=B, seed=0x5EED):
    from splendor.mcts import BatchedMCTS, HashEvaluator
    args = dict(numMCTSSims=sims, cpuct=2.5, fpu=0.3, prob_fullMCTS=1.0, ratio_fullMCTS=5, forced_playouts=False,
                dirichletAlpha=0.0, temperature=[1.25, 0.8], tempThreshold=10)
    return BatchedMCTS(e, batch, args, evaluator=HashEvaluator(e, mode=mode), seed=seed, mem_budget=MEM)


def host(pv):
    return {k: v.cpu().numpy() for k, v in pv.items()}


def check_shape_and_fill(pv, lines, depth, batch=B):
    """Shapes, codes in range, and the fill values in every entry at and past a line's length."""
    from splendor import _lib
    for k in ("action", "visits", "q", "prior"):
        assert pv[k].shape == (batch, lines, depth), k
    assert pv["length"].shape == pv["end"].shape == (batch, lines)
    ln, end = pv["length"], pv["end"]
    assert ((ln >= 0) & (ln <= depth)).all() and (end <= _lib.PV_END_NONE).all()
    np.testing.assert_array_equal(ln == 0, end == _lib.PV_END_NONE)
    np.testing.assert_array_equal(ln == depth, end == _lib.PV_END_DEPTH)
    unwritten = np.arange(depth)[None, None, :] >= ln[:, :, None]
    for k, v in FILL.items():
        assert (pv[k][unwritten] == v).all(), k
    assert (pv["action"][~unwritten] >= 0).all() and (pv["action"][~unwritten] < 409).all()
    assert (pv["visits"][~unwritten] >= 1).all()
    # the root's lines are ordered by (visits descending, action ascending), the written ones first
    v0, a0 = pv["visits"][:, :, 0].astype(np.int64), pv["action"][:, :, 0].astype(np.int64)
    both = ln[:, 1:] > 0
    key = v0 * 65536 + (65535 - a0)
    assert (key[:, :-1][both] > key[:, 1:][both]).all()
    assert (ln[:, :-1][both] > 0).all()


# ------------------------------------------------------------------ 1. the root level
@pytest.mark.parametrize("n", (2, 4))
def test_root_level_is_root_stats(engines, n):
    from splendor import _lib
    from splendor.review import rank_moves
    e = engines[n]
    m = handle(e, 64)
    m.get_action_prob(midgame_roots(e), keep_tree=False)
    lines = 4
    pv = host(m.principal_variations(lines, 1))
    check_shape_and_fill(pv, lines, 1)
    counts, qsa, _, _ = (t.cpu().numpy() for t in m.root_stats())
    ps = m.root_priors().cpu().numpy()
    order = rank_moves(counts)
    rows = np.arange(B)
    assert ((counts > 0).sum(1) >= lines).any()              # (some tree has every line)
    for k in range(lines):
        a = order[:, k]
        seen = counts[rows, a] > 0
        np.testing.assert_array_equal(pv["length"][:, k], seen.astype(np.int32))
        np.testing.assert_array_equal(pv["end"][:, k], np.where(seen, _lib.PV_END_DEPTH, _lib.PV_END_NONE))
        np.testing.assert_array_equal(pv["action"][seen, k, 0], a[seen])
        np.testing.assert_array_equal(pv["visits"][seen, k, 0], counts[rows, a][seen])
        assert pv["q"][seen, k, 0].tobytes() == qsa[rows, a][seen].tobytes()
        assert pv["prior"][seen, k, 0].tobytes() == ps[rows, a][seen].tobytes()


# ------------------------------------------------------------------ 2. deeper levels
@pytest.mark.parametrize("n,mode,sims", [(2, 1, 96), (2, 0, 96), (3, 1, 64)])
def test_deeper_levels_by_rerooting(engines, n, mode, sims):
    from splendor.review import rank_moves
    e = engines[n]
    roots = midgame_roots(e)
    lines, depth = 3, 6
    compared, longest, first = 0, 0, None
    for k in range(lines):
        m = handle(e, sims, mode)                            # the search is deterministic: the same trees
        m.get_action_prob(roots, keep_tree=False)
        pv_dev = m.principal_variations(lines, depth)
        pv = host(pv_dev)
        if first is None:
            first = pv
            check_shape_and_fill(pv, lines, depth)
        else:
            for key in pv:
                assert pv[key].tobytes() == first[key].tobytes(), key
        longest = max(longest, int(pv["length"].max()))
        parent = roots
        for d in range(1, depth):
            active = pv_dev["length"][:, k] > d
            if not bool(active.any()):
                break
            step = torch.where(pv_dev["length"][:, k] >= d, pv_dev["action"][:, k, d - 1],
                               torch.full_like(pv_dev["action"][:, k, 0], PASS))
            child = e.tree_step(parent, step.contiguous())
            m.set_roots_active(child, active.to(torch.uint8), keep_tree=True)
            counts, qsa, _, _ = (t.cpu().numpy() for t in m.root_stats())
            ps = m.root_priors().cpu().numpy()
            on = active.cpu().numpy()
            rows = np.flatnonzero(on)
            a = rank_moves(counts)[rows, 0]
            assert (counts[rows, a] > 0).all()
            np.testing.assert_array_equal(pv["action"][rows, k, d], a, err_msg=f"line {k} level {d}")
            np.testing.assert_array_equal(pv["visits"][rows, k, d], counts[rows, a], err_msg=f"line {k} level {d}")
            assert pv["q"][rows, k, d].tobytes() == qsa[rows, a].tobytes(), f"line {k} level {d}"
            assert pv["prior"][rows, k, d].tobytes() == ps[rows, a].tobytes(), f"line {k} level {d}"
            compared += len(rows)
            parent = child
    print(f"n={n} mode={mode} sims={sims}: longest line {longest}, {compared} entries below the root compared")
    assert longest >= 3 and compared > 0


# ------------------------------------------------------------------ 3. end codes
def test_end_codes_without_a_search(engines):
    from splendor import _lib
    e = engines[2]
    m = handle(e, 1)
    pv = host(m.principal_variations(3, 5))                  # before any set_roots: no root
    check_shape_and_fill(pv, 3, 5)
    assert (pv["end"] == _lib.PV_END_NONE).all() and (pv["length"] == 0).all()
    m.get_action_prob(midgame_roots(e), keep_tree=False)     # one simulation: the root is expanded,
    assert (m.headers()["root"] >= 0).all()                  # and nothing is visited
    pv = host(m.principal_variations(3, 5))
    check_shape_and_fill(pv, 3, 5)
    assert (pv["end"] == _lib.PV_END_NONE).all() and (pv["length"] == 0).all()


def test_end_codes_of_deep_trees(engines):
    from splendor import _lib
    e = engines[2]
    m = handle(e, 96, mode=1)
    m.get_action_prob(midgame_roots(e), keep_tree=False)
    counts = m.root_stats()[0].cpu().numpy()
    visited = (counts > 0).sum(1)
    # more lines than visited root edges: the trailing lines are NONE
    pv = host(m.principal_variations(16, 2))
    check_shape_and_fill(pv, 16, 2)
    assert (visited < 16).any()
    np.testing.assert_array_equal((pv["length"] > 0).sum(1), np.minimum(visited, 16))
    for t in range(B):
        assert (pv["end"][t, visited[t]:] == _lib.PV_END_NONE).all()
        assert (pv["end"][t, :visited[t]] != _lib.PV_END_NONE).all()
    assert (pv["end"] == _lib.PV_END_DEPTH).any()
    # the largest depth: every line ends by itself
    pv = host(m.principal_variations(3, 64))
    check_shape_and_fill(pv, 3, 64)
    assert (pv["length"] < 64).all() and (pv["length"][:, 0] >= 1).all()
    exists = pv["end"] != _lib.PV_END_NONE                   # (peaked priors: some trees visit one root edge only)
    np.testing.assert_array_equal(exists.sum(1), np.minimum(visited, 3))
    assert np.isin(pv["end"][exists], (_lib.PV_END_UNLINKED, _lib.PV_END_TERMINAL, _lib.PV_END_UNVISITED)).all()
    print("end codes at depth 64:", np.bincount(pv["end"].ravel(), minlength=5).tolist(),
          "longest", int(pv["length"].max()))


def test_terminal_lines_near_the_end_of_games(engines):
    """Roots one ply before the end of greedy-vs-greedy games: the move that ended the game leads
    to a terminal node of the tree."""
    from splendor import _lib
    from splendor.SplendorGame import SplendorGame
    from splendor.pit import BatchedPit, GreedyPlayer
    from splendor.review import replay
    g = SplendorGame(2)
    e = g.engine
    pit = BatchedPit(g, GreedyPlayer(), GreedyPlayer(), batch=B, seed=7)
    pit.playGames(B)
    rec = pit.record()
    rep = replay(e, rec)
    last = torch.from_numpy(rec["plies"].astype(np.int64) - 1).to(e.device)
    rows = torch.arange(B, device=e.device)
    roots = e.canonical(rep["boards"][rows, last].contiguous(), rep["mover"][rows, last].contiguous())
    m = handle(e, 64)
    m.get_action_prob(roots, keep_tree=False)
    pv_dev = m.principal_variations(8, 4)
    pv = host(pv_dev)
    check_shape_and_fill(pv, 8, 4)
    term = pv["end"] == _lib.PV_END_TERMINAL
    assert term.any()
    # a one-move line that ends TERMINAL: that move ends the game
    hit = 0
    for k in range(8):
        one = torch.from_numpy(term[:, k] & (pv["length"][:, k] == 1)).to(e.device)
        if not bool(one.any()):
            continue
        a = torch.where(one, pv_dev["action"][:, k, 0], torch.full_like(pv_dev["action"][:, k, 0], PASS))
        ended = (e.game_ended(e.tree_step(roots, a.contiguous())) != 0).any(1)
        assert bool(ended[one].all())
        hit += int(one.sum())
    assert hit > 0


# ------------------------------------------------------------------ 4. read-only
def test_pv_changes_nothing(engines):
    e = engines[2]
    m = handle(e, 64, mode=1)
    m.get_action_prob(midgame_roots(e), keep_tree=False)

    def snapshot():
        return (m.headers().tobytes(), m.tree_sizes().tobytes(), [t.cpu().numpy().tobytes() for t in m.root_stats()],
                m.pool_state())
    before = snapshot()
    one = host(m.principal_variations(3, 8))
    two = host(m.principal_variations(3, 8))
    assert snapshot() == before
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    # the optional outputs may be NULL
    action = torch.full((B, 3, 8), 99, dtype=torch.int16, device=e.device)
    length = torch.full((B, 3), 99, dtype=torch.int32, device=e.device)
    rc = m.L.spl_mcts_pv(m.h, 3, 8, ctypes.c_void_p(action.data_ptr()), None, None, None,
                         ctypes.c_void_p(length.data_ptr()), None, e._s())
    assert rc == 0
    np.testing.assert_array_equal(action.cpu().numpy(), one["action"])
    np.testing.assert_array_equal(length.cpu().numpy(), one["length"])
    assert snapshot() == before


# ------------------------------------------------------------------ 5. argument validation
def test_pv_argument_validation_on_a_live_handle(engines):
    from splendor import _lib
    e = engines[2]
    m = handle(e, 8)
    m.get_action_prob(midgame_roots(e), keep_tree=False)
    action = torch.full((B, 16, 64), 99, dtype=torch.int16, device=e.device)
    length = torch.full((B, 16), 99, dtype=torch.int32, device=e.device)
    pa, pl = ctypes.c_void_p(action.data_ptr()), ctypes.c_void_p(length.data_ptr())
    f = m.L.spl_mcts_pv
    for lines, depth in ((0, 8), (17, 8), (-1, 8), (3, 0), (3, 65), (3, -1)):
        assert f(m.h, lines, depth, pa, None, None, None, pl, None, e._s()) == _lib.EINVAL, (lines, depth)
    assert f(m.h, 3, 8, None, None, None, None, pl, None, e._s()) == _lib.EINVAL
    assert f(m.h, 3, 8, pa, None, None, None, None, None, e._s()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((action == 99).all()) and bool((length == 99).all())      # nothing was launched
    assert f(m.h, 16, 64, pa, None, None, None, pl, None, e._s()) == 0    # the largest legal call
    torch.cuda.synchronize()
    assert bool((length <= 64).all()) and bool((length >= 0).all())
    for bad in ((0, 8), (17, 8), (3, 0), (3, 65)):
        with pytest.raises(_lib.EngineError):
            m.principal_variations(*bad)


# ------------------------------------------------------------------ 6. replay
@pytest.fixture(scope="module")
def records():
    from splendor.SplendorGame import SplendorGame
    from splendor.pit import BatchedPit, GreedyPlayer, RandomPlayer
    out = {}
    for n in (2, 3):
        g = SplendorGame(n)
        pit = BatchedPit(g, GreedyPlayer(), RandomPlayer(), batch=8, seed=21, game_base=3)
        totals = pit.playGames(8)
        out[n] = (g, pit.record(), dict(pit.last), totals)
    return out


@pytest.mark.parametrize("n", (2, 3))
def test_replay_reproduces_the_record(records, n):
    from splendor.review import RECORD_KEYS, replay
    g, rec, last, _ = records[n]
    e = g.engine
    assert set(rec) == set(RECORD_KEYS) and set(last) == {"game", "one_vs_two", "result", "plies", "score", "actions"}
    for k in last:
        np.testing.assert_array_equal(rec[k], last[k], err_msg=k)
    assert (int(rec["seed"]), int(rec["game_base"]), int(rec["n"]), int(rec["rules"]), int(rec["token_limit"])) == \
        (21, 3, n, 0, 10)
    rep = replay(e, rec)
    P = int(rec["plies"].max())
    assert rep["boards"].shape == (8, P, e.rows, 7) and rep["final"].shape == (8, e.rows, 7)
    np.testing.assert_array_equal(e.score(rep["final"]).cpu().numpy(), rec["score"])
    np.testing.assert_array_equal(e.game_ended(rep["final"]).cpu().numpy(), rec["result"])
    np.testing.assert_array_equal(rep["live"].sum(1).cpu().numpy(), rec["plies"])
    np.testing.assert_array_equal(rep["mover"].cpu().numpy(), np.tile(np.arange(P) % n, (8, 1)))
    deal = e.new_state(8)
    e.init(deal, None, seed=21, stream=0xFFFFFFFF, board_base=3)
    assert torch.equal(rep["boards"][:, 0], deal)
    # no position before a game's last is finished, and the boards past its end are not written
    live = rep["live"]
    assert not bool((e.game_ended(rep["boards"][live].contiguous()) != 0).any())
    assert not bool(rep["boards"][~live].any())
    # a subset in any order, one game at a time: the same positions
    sub = replay(e, rec, games=[5, 2, 6])
    for i, gme in enumerate((5, 2, 6)):
        p = int(rec["plies"][gme])
        assert torch.equal(sub["boards"][i, :p], rep["boards"][gme, :p])
        assert torch.equal(sub["final"][i], rep["final"][gme])


def test_replay_raises_on_a_record_that_disagrees(records):
    from splendor.SplendorGame import SplendorGame
    from splendor.review import replay
    g, rec, _, _ = records[2]
    e = g.engine

    def altered(key, index, value):
        r = {k: np.array(v) for k, v in rec.items()}
        r[key][index] = value
        return r
    with pytest.raises(ValueError, match="not legal"):       # nobody can buy a card on the first move
        replay(e, altered("actions", (0, 0), 0))
    p = int(rec["plies"][4])
    with pytest.raises(ValueError):                          # the last move replaced by another game's
        replay(e, altered("actions", (4, p - 1), PASS))
    with pytest.raises(ValueError, match="score"):
        replay(e, altered("score", (1, 0), int(rec["score"][1, 0]) + 1))
    with pytest.raises(ValueError, match="result"):
        replay(e, altered("result", 2, -rec["result"][2]))
    with pytest.raises(ValueError, match="another ply"):
        replay(e, altered("plies", 6, int(rec["plies"][6]) - 1))
    with pytest.raises(ValueError, match="engine has"):
        replay(SplendorGame(3).engine, rec)
    replay(e, rec)                                           # the record itself still replays


# ------------------------------------------------------------------ 7. review end to end
def test_review_end_to_end(engines):
    from splendor.SplendorGame import SplendorGame
    from splendor.env import unpack_mask
    from splendor.pit import BatchedPit, GreedyPlayer, RandomPlayer
    from splendor.playout import PlayoutEvaluator
    from splendor.review import replay, review
    g = SplendorGame(2)
    e = g.engine
    pit = BatchedPit(g, GreedyPlayer(), RandomPlayer(), batch=4, seed=9)
    pit.playGames(4)
    rec = pit.record()
    args = dict(numMCTSSims=16, cpuct=2.5, fpu=0.3)
    lines, depth = 3, 4
    # (128 trees at a time: several batches, the last one padded; a handle's fixed cost is ~2 MiB
    # per tree, so 1 GiB leaves the pools room; a capacity warning is an error here)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*capacity events.*")
        runs = [review(g, PlayoutEvaluator(e, playouts=2, seed=5), rec, args, lines=lines, depth=depth, batch=128,
                       mem_budget=1 << 30) for _ in range(2)]
    out = runs[0]
    N = int(rec["plies"].sum())
    for k, v in out.items():
        assert v.shape[0] == N, k
        np.testing.assert_array_equal(v, runs[1][k], err_msg=k)          # (NaNs compare equal here)
    want = [(i, p) for i in range(4) for p in range(int(rec["plies"][i]))]
    assert list(zip(out["game"].tolist(), out["ply"].tolist())) == want
    np.testing.assert_array_equal(out["mover"], out["ply"] % 2)
    np.testing.assert_array_equal(out["played"], rec["actions"][out["game"], out["ply"]])
    assert (out["value"] >= -1).all() and (out["value"] <= 1).all()
    assert (out["entropy"] >= 0).all() and (out["entropy"] > 0).any()
    assert (out["visits"] == 15).all()                       # 16 simulations: the first expands the root
    assert out["scores"].shape == (N, 2) and (out["scores"] >= 0).all()
    np.testing.assert_array_equal(out["scores"][out["ply"] == 0], 0)
    # the played move's rank, recounted from the counts
    c, a = out["counts"], out["played"]
    cp = c[np.arange(N), a]
    rank = (c > cp[:, None]).sum(1) + ((c == cp[:, None]) & (np.arange(409)[None, :] < a[:, None])).sum(1)
    np.testing.assert_array_equal(out["played_rank"], rank)
    np.testing.assert_array_equal(out["played_visits"], cp)
    np.testing.assert_array_equal(np.isnan(out["q_loss"]), cp == 0)
    np.testing.assert_array_equal(out["pv_action"][:, 0, 0], out["best"])
    np.testing.assert_array_equal(out["pv_visits"][:, 0, 0], out["best_visits"])
    assert out["pv_q"][:, 0, 0].tobytes() == out["best_q"].tobytes()
    # every move of every line is legal where it is played
    rep = replay(e, rec)
    idx = rep["live"].nonzero()
    canon = e.canonical(rep["boards"][idx[:, 0], idx[:, 1]].contiguous(), rep["mover"][idx[:, 0], idx[:, 1]].contiguous())
    assert (out["pv_length"][:, 0] >= 1).all()
    for k in range(lines):
        boards = canon
        for d in range(depth):
            on = torch.from_numpy(out["pv_length"][:, k] > d).to(e.device)
            if not bool(on.any()):
                break
            act = torch.from_numpy(out["pv_action"][:, k, d]).to(e.device)
            valid = unpack_mask(e.valid_moves(boards))
            assert bool(valid.gather(1, act.long().clamp(0, 408).unsqueeze(1)).squeeze(1)[on].all()), (k, d)
            boards = e.tree_step(boards, torch.where(on, act, torch.full_like(act, PASS)).contiguous())
