"""spl_playout_seq on the device, bit for bit against spl_playout: the stream base read from
the device counter, the rows given as the search's segmented leaf list, the evaluator on both
paths inside the search, self-play under graph capture against the eager run, and the rollout
bootstrap of Coach.learn.

Workgroup geometry with a list: 64 / P consecutive list entries per workgroup, so at B = 150
(segments of 64, 64 and 22 rows) P = 1 puts entries of several segments into one workgroup,
P = 3 gives 21 entries per workgroup (they straddle segment boundaries, one idle lane) and
P = 64 one entry per workgroup. The count scan covers 256 segments per pass: B = 19,200 (300
segments) takes two."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MEM = 1 << 28
SEED, BASE = 0x1234ABCD5EED, 0xFFFFFFC0                     # (board ids wrap past 2^32)
SENT = -7


@functools.lru_cache(maxsize=None)
def engine(n):
    from splendor.env import SplendorEngine
    return SplendorEngine(n, device="cuda")


@functools.lru_cache(maxsize=None)
def leaves(n, B):
    """B canonical mid-game boards (20 n random moves from the deal, no game over); shared
    and left unchanged."""
    from splendor.env import RolloutBatch
    e = engine(n)
    rb = RolloutBatch(e, B, seed=0xC0FFEE)
    rb.run(20 * n, masks=False)
    assert int(rb.games.sum()) == 0                          # (no game is over: nothing re-dealt)
    return e.canonical(rb.state, rb.player).contiguous()


def sentinels(e, B, Pn):
    dev = e.device
    return {"result": torch.full((B, e.n), float(SENT), dtype=torch.float32, device=dev),
            "pi": torch.full((B, 409), float(SENT), dtype=torch.float32, device=dev),
            "steps": torch.full((B, Pn), SENT, dtype=torch.int32, device=dev)}


def same(got, want):
    for k in ("result", "pi", "steps"):
        assert torch.equal(got[k], want[k]), k
    assert int(got["unfinished"].item()) == int(want["unfinished"].item()) == 0


def seq_tensor(e, c):
    return torch.tensor([c - (1 << 32) if c >= 1 << 31 else c], dtype=torch.int32, device=e.device)


# ------------------------------------------------------------------ 1. sequence = host step
@pytest.mark.parametrize("Pn", (1, 3))
@pytest.mark.parametrize("n", (2, 3, 4))
def test_sequence_is_the_host_step(n, Pn):
    e, B = engine(n), 70
    st = leaves(n, B)
    flags = torch.from_numpy((np.arange(B) % 5 != 2).astype(np.uint8)).to(e.device)
    off = flags == 0
    policy = "uniform" if Pn == 1 else "buy_first"
    kw = dict(active=flags, policy=policy, playouts=Pn, seed=SEED, board_base=BASE, pi=True, steps=True)
    seen = []
    for c, step0 in ((0, 0), (5, 256 * 5), ((1 << 23) - 1, 256 * ((1 << 23) - 1)), (1 << 23, 0)):
        want = e.playout(st, step0=step0, out=sentinels(e, B, Pn), **kw)
        seq = seq_tensor(e, c)
        got = e.playout_seq(st, seq, out=sentinels(e, B, Pn), **kw)
        torch.cuda.synchronize()
        same(got, want)
        assert int(seq.item()) == c                          # the kernel only reads the counter
        for k in ("result", "pi", "steps"):
            assert bool((got[k][off] == SENT).all()), k      # inactive rows keep every byte
            assert bool((got[k][~off] != SENT).all()), k
        seen.append(got["steps"].clone())
    assert torch.equal(seen[0], seen[3])                     # 2^23 wraps to stream base 0
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ------------------------------------------------------------------ 2. the list
def make_list(B, seg_rows, rng):
    """leaf_index / leaf_count from per-segment row lists, each shuffled; the unused slots of
    leaf_index hold unlisted rows, so an entry read past a count would touch a sentinel."""
    nseg = (B + 63) // 64
    listed = np.zeros(B, bool)
    for rows in seg_rows.values():
        listed[np.asarray(rows, int)] = True
    spare = np.flatnonzero(~listed)
    index = (spare[np.arange(B) % len(spare)] if len(spare) else np.zeros(B, int)).astype(np.int32)
    count = np.zeros(nseg, np.int32)
    for j, rows in seg_rows.items():
        rows = np.asarray(rows, np.int32)
        assert ((rows >= 64 * j) & (rows < min(64 * j + 64, B))).all() and len(set(rows.tolist())) == len(rows)
        index[64 * j:64 * j + len(rows)] = rng.permutation(rows)
        count[j] = len(rows)
    return index, count, listed


def check_list(e, st, Pn, seg_rows, rng, c=7):
    B, dev = st.shape[0], e.device
    index, count, listed = make_list(B, seg_rows, rng)
    kw = dict(policy="buy_first", playouts=Pn, seed=SEED, board_base=BASE, pi=True, steps=True)
    want = e.playout(st, active=torch.from_numpy(listed.astype(np.uint8)).to(dev), step0=256 * c,
                     out=sentinels(e, B, Pn), **kw)
    got = e.playout_seq(st, seq_tensor(e, c), index=torch.from_numpy(index).to(dev),
                        count=torch.from_numpy(count).to(dev), out=sentinels(e, B, Pn), **kw)
    torch.cuda.synchronize()
    same(got, want)
    off = torch.from_numpy(~listed).to(dev)
    for k in ("result", "pi", "steps"):
        assert bool((got[k][off] == SENT).all()), k          # every other row keeps its sentinel
        assert bool((got[k][~off] != SENT).all()), k
    return got


@pytest.mark.parametrize("Pn", (1, 3, 64))
def test_list_rows_equal_flagged_rows(Pn):
    n, B = 2, 150
    e, st = engine(n), leaves(2, 150)
    rng = np.random.default_rng(Pn)
    pick = lambda lo, hi, k: rng.choice(np.arange(lo, hi), k, replace=False)
    check_list(e, st, Pn, {0: pick(0, 64, 5), 2: np.arange(128, 150)}, rng)          # counts (5, 0, 22)
    check_list(e, st, Pn, {1: np.arange(64, 128)}, rng)                              # counts (0, 64, 0)
    got = check_list(e, st, Pn, {}, rng)                                             # nothing listed
    for k in ("result", "pi", "steps"):
        assert bool((got[k] == SENT).all()), k
    check_list(e, st, Pn, {0: np.arange(64), 1: np.arange(64, 128), 2: np.arange(128, 150)}, rng)   # every row
    check_list(e, st, Pn, {0: pick(0, 64, 44), 1: pick(64, 128, 43), 2: pick(128, 150, 9)}, rng)    # a search's share


def test_list_over_many_segments():
    """300 segments: the count scan takes a second pass; one leaf in every seventh segment
    and a full last segment, so workgroup 0 gathers its entries from 43 segments apart."""
    n, B = 2, 19200
    e, st = engine(n), leaves(2, 19200)
    rng = np.random.default_rng(5)
    seg_rows = {j: [64 * j + int(rng.integers(64))] for j in range(0, 299, 7)}
    seg_rows[299] = np.arange(64 * 299, B)
    check_list(e, st, 1, seg_rows, rng)


# ------------------------------------------------------------------ 3. inside the search
def searched(wrap):
    from splendor.mcts import BatchedMCTS
    from splendor.playout import PlayoutEvaluator
    n, B, sims, seed = 2, 8, 16, 21
    e = engine(n)
    ev = PlayoutEvaluator(e, playouts=2, policy="buy_first", seed=seed, board_base=3)
    used = []

    def plain(state, mask, valid):                           # no `indexed`: the flag path
        used.append(1)
        return ev(state, mask, valid)
    m = BatchedMCTS(e, B, dict(numMCTSSims=sims, cpuct=2.5, fpu=0.3), evaluator=plain if wrap else ev, seed=seed,
                    mem_budget=MEM)
    roots = e.init(e.new_state(B), seed=seed)
    _, q, _, counts = m.get_action_prob(roots)
    assert ev.calls == sims and len(used) == (sims if wrap else 0)
    assert m.capacity_events() == {"prunes": 0, "resets": 0, "unexpanded": 0}
    assert bool((counts.sum(1) == sims - 1).all())
    if not wrap:
        assert int(m.leaf_count.sum()) > 0                   # the list path wrote its counts
    return counts, q


def test_list_and_flag_paths_search_alike():
    (c0, q0), (c1, q1) = searched(False), searched(True)
    assert torch.equal(c0, c1) and torch.equal(q0, q1)


# ------------------------------------------------------------------ 4. capture
SP_ARGS = dict(numMCTSSims=4, cpuct=2.5, fpu=0.3, prob_fullMCTS=1.0, ratio_fullMCTS=5, forced_playouts=False,
               dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
HDR = ("player", "episode_step", "move_no", "game_no", "games_done", "moves", "sims_done")


def rollout_selfplay(B=8, playouts=2, seed=11, **kw):
    from splendor.playout import PlayoutEvaluator
    from splendor.selfplay import SelfPlay
    e = engine(2)
    ev = PlayoutEvaluator(e, playouts=playouts, policy="buy_first", seed=seed, board_base=0)
    sp = SelfPlay(e, B, SP_ARGS, evaluator=ev, dirichlet_noise=True, seed=seed, mem_budget=MEM,
                  out_cap=B * 126 * 8, **kw)
    sp.reset()
    return sp, ev


def test_captured_selfplay_is_the_eager_run():
    """A 2-player game has at most 124 plies of 4 simulations each: k = 645 iterations end a
    game on every tree, and (k - 1) = 80 x 8 + 4 replays both graphs."""
    k = 645
    eager, ev0 = rollout_selfplay()
    eager.run(k, use_graph=False)
    graphed, ev1 = rollout_selfplay()
    graphed.run(k, use_graph=True)
    assert graphed.graph is not None and graphed.graph_k is not None
    torch.cuda.synchronize()
    assert ev0.calls == k and ev1.calls == k
    h0, h1 = eager.headers().copy(), graphed.headers().copy()
    assert h0["games_done"].min() >= 1
    for f in HDR:
        np.testing.assert_array_equal(h0[f], h1[f], err_msg=f)
    x0, x1 = ({key: v.cpu().numpy() for key, v in sp.drain().items()} for sp in (eager, graphed))
    assert len(x0["meta"]) > 0
    # the device queue order is nondeterministic: order both sides by their meta columns
    o0, o1 = np.lexsort(x0["meta"].T[::-1]), np.lexsort(x1["meta"].T[::-1])
    for key in x0:
        np.testing.assert_array_equal(x0[key][o0], x1[key][o1], err_msg=key)
    for sp in (eager, graphed):
        assert sp.capacity_events() == {"prunes": 0, "resets": 0, "unexpanded": 0}


# ------------------------------------------------------------------ 5. Coach
def coach_args(tmp_path, **kw):
    return dict(SP_ARGS, numIters=2, numEps=8, numItersHistory=3, arenaCompare=2, updateThreshold=0.55,
                checkpoint=str(tmp_path), **kw)


def test_coach_bootstraps_from_rollout_selfplay(tmp_path):
    from splendor import coach as coach_mod
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame
    from splendor.examples import FIELDS
    from splendor.playout import PlayoutEvaluator
    from splendor.selfplay import SelfPlay
    g = SplendorGame(2)
    nn = NNetWrapper(g, dict(epochs=1, batch_size=32))
    seed, B = 4, 8
    c = coach_mod.Coach(g, nn, coach_args(tmp_path, bootstrap_iters=1), batch=B, seed=seed, mem_budget=MEM)
    net_ev, rules = c.sp.evaluator, g.engine.rules
    assert not isinstance(net_ev, PlayoutEvaluator)
    played, inner = [], c.executeIteration

    def spy(*a, **k):
        played.append(c.sp.evaluator)
        return inner(*a, **k)
    c.executeIteration = spy
    hist = c.learn()
    assert len(hist) == 2 and len(played) == 2
    assert isinstance(played[0], PlayoutEvaluator) and (played[0].playouts, played[0].policy) == (4, "buy_first")
    assert (played[0].seed, played[0].board_base) == (seed, 0)
    assert type(played[1]) is type(net_ev) and not isinstance(c.sp.evaluator, PlayoutEvaluator)
    assert len(c.trainExamplesHistory.iters) == 2
    assert g.engine.rules == rules and c.sp.rules == rules
    assert c.use_rollout_selfplay() is played[0]             # one evaluator for every bootstrap iteration
    c.refresh_network()
    # iteration 1 again on a bare handle, driven as executeEpisodes drives it
    sp = SelfPlay(g.engine, B, c.args, evaluator=PlayoutEvaluator(g.engine, 4, "buy_first", seed=seed),
                  dirichlet_noise=True, seed=seed, mem_budget=MEM)
    sp.reset()
    sp.reset()
    parts, done, start = [], 0, sp.stats()["games_done"]
    while done < 8:
        sp.run(32, use_graph=False)
        ex = sp.drain()
        if ex["board"].shape[0]:
            parts.append(ex)
        done = sp.stats()["games_done"] - start
    ex = coach_mod.expand_symmetries(g.engine, {k: torch.cat([p[k] for p in parts]) for k in parts[0]})
    first = c.trainExamplesHistory.iters[0]
    assert len(first) == ex["board"].shape[0] > 0

    def records(col):
        """Every example as one byte string over all fields, sorted (the queue order is not defined)."""
        cols = [col(f).cpu().contiguous().numpy() for f in FIELDS]
        return sorted(b"".join(a[i].tobytes() for a in cols) for i in range(len(cols[0])))
    assert records(lambda f: getattr(first, f)) == records(lambda f: ex[f])


def test_coach_without_bootstrap_builds_no_rollout_evaluator(tmp_path, monkeypatch):
    from splendor import coach as coach_mod
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame

    def no_rollout(*a, **k):
        raise AssertionError("a PlayoutEvaluator was built without bootstrap_iters")
    monkeypatch.setattr(coach_mod, "PlayoutEvaluator", no_rollout)
    g = SplendorGame(2)
    nn = NNetWrapper(g, dict(epochs=1, batch_size=32))
    c = coach_mod.Coach(g, nn, dict(coach_args(tmp_path), numIters=1), batch=8, seed=4, mem_budget=MEM)
    assert len(c.learn()) == 1
    with pytest.raises(AssertionError):
        c.use_rollout_selfplay()


# ------------------------------------------------------------------ 6. set_evaluator
class Counting:
    """HashEvaluator that counts its executions on the device (a captured add)."""

    def __init__(self, e):
        from splendor.mcts import HashEvaluator
        self.inner = HashEvaluator(e)
        self.n = torch.zeros(1, dtype=torch.int32, device=e.device)

    def __call__(self, state, mask, valid):
        self.n += 1
        return self.inner(state, mask, valid)


def test_set_evaluator_drops_the_graphs(tmp_path, monkeypatch):
    from splendor import coach as coach_mod
    from splendor.SplendorGame import SplendorGame
    g = SplendorGame(2)
    c = coach_mod.Coach(g, None, coach_args(tmp_path), batch=8, seed=4, mem_budget=MEM)
    old = Counting(g.engine)
    c.sp.set_evaluator(old)
    c.sp.run(10, use_graph=True)                             # 1 eager + 8 in one replay + 1 single replay
    assert c.sp.graph is not None and c.sp.graph_k is not None
    assert int(old.n.item()) == 10
    new = Counting(g.engine)
    monkeypatch.setattr(coach_mod, "evaluator_for", lambda *a, **k: new)
    c.refresh_network()
    assert c.sp.evaluator is new and c.sp.graph is None and c.sp.graph_k is None
    c.sp.run(10, use_graph=True)
    torch.cuda.synchronize()
    assert int(new.n.item()) == 10 and int(old.n.item()) == 10
