"""spl_playout_mix on the device: the blend against the host formula over spl_playout_seq's
means, lambda = 0 as a launch that writes nothing, the leaf list against the flags, the mixed
evaluator inside the search (against the plain network search at lambda = 0, list against flag
path, against the playout evaluator at lambda = 1), self-play under graph capture with lambda
changed between replays, Coach's rollout_mix schedule and the pit's MixedPlayer.

The boards, lists and self-play arguments are test_playout_seq_gpu's (shared, unchanged)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_playout_seq_gpu as S  # noqa: E402  (fixtures only: engine, leaves, make_list, seq_tensor, SP_ARGS)

pytestmark = pytest.mark.gpu

MEM, SEED, BASE, SENT = S.MEM, S.SEED, S.BASE, S.SENT
NO_EVENTS = {"prunes": 0, "resets": 0, "unexpanded": 0}


def lam_tensor(e, x):
    return torch.tensor([x], dtype=torch.float32, device=e.device)


def dev_u8(e, a):
    return torch.from_numpy(np.asarray(a).astype(np.uint8)).to(e.device)


def blend(lam, v, m):
    """The header's formula in numpy float32: two products and one sum, no contraction."""
    lam = np.float32(lam)
    out = (np.float32(1) - lam) * v + lam * m
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------ 1. the blend
@pytest.mark.parametrize("Pn", (1, 3))
@pytest.mark.parametrize("n", (2, 3, 4))
def test_blend_is_the_host_formula(n, Pn):
    e, B = S.engine(n), 70
    st = S.leaves(n, B)
    on = np.arange(B) % 5 != 2
    flags = dev_u8(e, on)
    kw = dict(active=flags, policy="uniform" if Pn == 1 else "buy_first", playouts=Pn, seed=SEED, board_base=BASE)
    v0 = (np.random.default_rng(100 * n + Pn).random((B, n), dtype=np.float32) * np.float32(2) - np.float32(1))
    v0 = np.clip(v0, np.float32(-0.999), np.float32(0.999))
    assert v0.dtype == np.float32 and np.abs(v0).max() < 1
    means = []
    for c in (0, 5, 1 << 23):
        seq = S.seq_tensor(e, c)
        m = e.playout_seq(st, seq, **kw)["result"].cpu().numpy()
        assert np.abs(m[on]).max() > 0                        # (something to mix in)
        means.append(m)
        for lam in (0.25, 0.5, 1.0):
            v = torch.from_numpy(v0).to(e.device)
            got, unfinished = e.playout_mix(st, seq, lam_tensor(e, lam), v, **kw)
            torch.cuda.synchronize()
            assert got is v
            g = got.cpu().numpy()
            print(f"n={n} P={Pn} c={c} lam={lam}: max |got - host| = {np.abs(g[on] - blend(lam, v0, m)[on]).max()}")
            assert np.array_equal(g[on], blend(lam, v0, m)[on])
            assert g[~on].tobytes() == v0[~on].tobytes()      # inactive rows keep every byte
            assert not np.array_equal(g[on], v0[on])
            if lam == 1.0:
                assert np.array_equal(g[on], m[on])
            assert int(unfinished.item()) == 0
            assert int(seq.item()) == c                       # the kernel only reads the counter
    assert np.array_equal(means[0], means[2]) and not np.array_equal(means[0], means[1])   # 2^23 wraps to base 0


# ------------------------------------------------------------------ 2. lambda = 0
@pytest.mark.parametrize("rows", ("all", "flags", "list"))
def test_zero_lambda_writes_nothing(rows):
    """max_steps = 1 ends no playout: a launch that ran any would count it in `unfinished` (the
    control at lambda = 0.5 does), so unfinished == 0 shows the workgroups left before playing."""
    n, B, c = 2, 150, 9
    e, st = S.engine(n), S.leaves(n, B)
    rng = np.random.default_rng(3)
    how = {}
    if rows == "flags":
        how = dict(active=dev_u8(e, np.arange(B) % 3 != 1))
    elif rows == "list":
        index, count, _ = S.make_list(B, {0: np.arange(64), 1: np.arange(64, 128), 2: np.arange(128, 150)}, rng)
        how = dict(index=torch.from_numpy(index).to(e.device), count=torch.from_numpy(count).to(e.device))
    v0 = rng.integers(0, 256, B * n * 4, dtype=np.uint8)     # any bytes (NaN patterns included)
    seq = S.seq_tensor(e, c)
    for P in (1, 4):
        kw = dict(policy="buy_first", playouts=P, seed=SEED, board_base=BASE, max_steps=1, **how)
        for lam in (0.0, -0.0, float("nan"), -2.5):
            v = torch.from_numpy(v0.copy()).to(e.device).view(torch.float32).view(B, n)
            _, unfinished = e.playout_mix(st, seq, lam_tensor(e, lam), v, **kw)
            torch.cuda.synchronize()
            assert v.cpu().numpy().tobytes() == v0.tobytes(), lam
            assert int(unfinished.item()) == 0, lam
            assert int(seq.item()) == c
        v = torch.zeros((B, n), dtype=torch.float32, device=e.device)
        _, unfinished = e.playout_mix(st, seq, lam_tensor(e, 0.5), v, **kw)
        torch.cuda.synchronize()
        assert int(unfinished.item()) > 0                     # the control: these launches do play
        v.fill_(0.25)
        _, unfinished = e.playout_mix(st, seq, lam_tensor(e, 7.0), v, **dict(kw, max_steps=None))
        m = e.playout_seq(st, seq, out={"result": torch.full_like(v, 0.25)}, **dict(kw, max_steps=None))["result"]
        torch.cuda.synchronize()
        assert int(unfinished.item()) == 0 and torch.equal(v, m)     # 7 clamps to 1: v is the mean


# ------------------------------------------------------------------ 3. the list
def check_list(e, st, Pn, seg_rows, rng, c=7, lam=0.5):
    B, dev = st.shape[0], e.device
    index, count, listed = S.make_list(B, seg_rows, rng)
    kw = dict(policy="buy_first", playouts=Pn, seed=SEED, board_base=BASE)
    flags = dev_u8(e, listed)
    start = lambda: torch.full((B, e.n), float(SENT), dtype=torch.float32, device=dev)   # noqa: E731
    m = e.playout_seq(st, S.seq_tensor(e, c), active=flags, **kw)["result"].cpu().numpy()
    want, u0 = e.playout_mix(st, S.seq_tensor(e, c), lam_tensor(e, lam), start(), active=flags, **kw)
    got, u1 = e.playout_mix(st, S.seq_tensor(e, c), lam_tensor(e, lam), start(), index=torch.from_numpy(index).to(dev),
                            count=torch.from_numpy(count).to(dev), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert int(u0.item()) == int(u1.item()) == 0
    g = got.cpu().numpy()
    assert bool((g[~listed] == SENT).all())                   # every other row keeps its sentinel
    assert bool((g[listed] != SENT).all())
    assert np.array_equal(g[listed], blend(lam, np.full_like(m, SENT), m)[listed])
    return g


@pytest.mark.parametrize("Pn", (1, 3, 64))
def test_list_rows_equal_flagged_rows(Pn):
    n, B = 2, 150
    e, st = S.engine(n), S.leaves(2, 150)
    rng = np.random.default_rng(Pn)
    pick = lambda lo, hi, k: rng.choice(np.arange(lo, hi), k, replace=False)   # noqa: E731
    check_list(e, st, Pn, {0: pick(0, 64, 5), 2: np.arange(128, 150)}, rng)          # counts (5, 0, 22)
    check_list(e, st, Pn, {1: np.arange(64, 128)}, rng)                              # counts (0, 64, 0)
    got = check_list(e, st, Pn, {}, rng)                                             # nothing listed
    assert bool((got == SENT).all())
    check_list(e, st, Pn, {0: np.arange(64), 1: np.arange(64, 128), 2: np.arange(128, 150)}, rng)   # every row
    check_list(e, st, Pn, {0: pick(0, 64, 44), 1: pick(64, 128, 43), 2: pick(128, 150, 9)}, rng)    # a search's share


def test_list_over_many_segments():
    """300 segments: the count scan takes a second pass (test_playout_seq_gpu's list)."""
    n, B = 2, 19200
    e, st = S.engine(n), S.leaves(2, 19200)
    rng = np.random.default_rng(5)
    seg_rows = {j: [64 * j + int(rng.integers(64))] for j in range(0, 299, 7)}
    seg_rows[299] = np.arange(64 * 299, B)
    check_list(e, st, 1, seg_rows, rng)


# ------------------------------------------------------------------ 4. inside the search
@functools.lru_cache(maxsize=None)
def network(seed=0):
    from splendor.nnet import random_net
    return random_net(2, seed=seed, device="cuda")


def leaf_evaluator(B):
    from splendor.nnet import LeafEvaluator
    return LeafEvaluator(S.engine(2), network(), B, use_graph=False)


def searched(lam, wrap=False):
    """16 simulations on 8 trees; lam None: the plain network evaluator (the staged path)."""
    from splendor.mcts import BatchedMCTS
    from splendor.playout import MixedEvaluator
    n, B, sims, seed = 2, 8, 16, 21
    e = S.engine(n)
    net = leaf_evaluator(B)
    ev = net if lam is None else MixedEvaluator(e, net, playouts=2, policy="buy_first", lam=lam, seed=seed,
                                                board_base=3)
    used = []

    def plain(state, mask, valid):                           # no `indexed`: the flag path
        used.append(1)
        return ev(state, mask, valid)
    m = BatchedMCTS(e, B, dict(numMCTSSims=sims, cpuct=2.5, fpu=0.3), evaluator=plain if wrap else ev, seed=seed,
                    mem_budget=MEM)
    roots = e.init(e.new_state(B), seed=seed)
    _, q, _, counts = m.get_action_prob(roots)
    assert m.capacity_events() == NO_EVENTS
    assert bool((counts.sum(1) == sims - 1).all())
    assert len(used) == (sims if wrap else 0)
    if lam is None:
        assert m._staged_select                              # the network alone reads the staged buffer
    else:
        assert ev.calls == sims and ev.unfinished == 0
        assert not m._staged_select
        if not wrap:
            assert int(m.leaf_count.sum()) > 0               # the list path wrote its counts
    return counts, q


def test_zero_lambda_search_is_the_network_search():
    (c0, q0), (c1, q1) = searched(None), searched(0.0)
    assert torch.equal(c0, c1) and torch.equal(q0, q1)


def test_list_and_flag_paths_search_alike():
    (c0, q0), (c1, q1) = searched(0.5), searched(0.5, wrap=True)
    assert torch.equal(c0, c1) and torch.equal(q0, q1)
    cn, qn = searched(None)
    assert not torch.equal(q0, qn)                           # (the playouts do change the values)


def test_lambda_one_values_are_the_playout_evaluators():
    from splendor.playout import MixedEvaluator, PlayoutEvaluator
    n, B, seed = 2, 70, 21
    e, st = S.engine(n), S.leaves(n, B)
    on = np.arange(B) % 5 != 2
    flags, mask = dev_u8(e, on), e.valid_moves(st)
    net_pi, net_v = (t.clone() for t in leaf_evaluator(B)(st, mask, flags))
    mixed = MixedEvaluator(e, leaf_evaluator(B), playouts=2, policy="buy_first", lam=1.0, seed=seed, board_base=3)
    rollout = PlayoutEvaluator(e, playouts=2, policy="buy_first", seed=seed, board_base=3)
    seen = []
    for call in range(2):
        pi, v = mixed(st, mask, flags)
        _, want = rollout(st, mask, flags)
        torch.cuda.synchronize()
        assert mixed.calls == rollout.calls == call + 1
        assert torch.equal(pi, net_pi)
        assert torch.equal(v[flags.bool()], want[flags.bool()])
        assert torch.equal(v[~flags.bool()], net_v[~flags.bool()])    # rows that did not run: the network's
        seen.append(v.clone())
    assert not torch.equal(seen[0], seen[1])                 # the second call drew new streams


# ------------------------------------------------------------------ 5. capture
def mixed_selfplay(B=8, playouts=2, seed=11):
    from splendor.playout import MixedEvaluator
    from splendor.selfplay import SelfPlay
    e = S.engine(2)
    ev = MixedEvaluator(e, leaf_evaluator(B), playouts=playouts, policy="buy_first", lam=0.5, seed=seed)
    sp = SelfPlay(e, B, S.SP_ARGS, evaluator=ev, dirichlet_noise=True, seed=seed, mem_budget=MEM,
                  out_cap=B * 126 * 16)
    sp.reset()
    return sp, ev


def test_lambda_changes_under_captured_selfplay():
    """k = 645 as test_captured_selfplay_is_the_eager_run: the first graphed run is the eager
    iteration, 80 replays of the 8-iteration graph and 4 single replays; the second, after the
    lambda write, 80 and 5 replays of the same two graphs."""
    k = 645
    eager, ev0 = mixed_selfplay()
    eager.run(k, use_graph=False)
    ev0.lam = 0.25
    eager.run(k, use_graph=False)
    graphed, ev1 = mixed_selfplay()
    graphed.run(k, use_graph=True)
    g1, gk = graphed.graph, graphed.graph_k
    assert g1 is not None and gk is not None
    ev1.lam = 0.25
    assert graphed.graph is g1 and graphed.graph_k is gk
    graphed.run(k, use_graph=True)
    assert graphed.graph is g1 and graphed.graph_k is gk     # the lambda write dropped no graph
    torch.cuda.synchronize()
    assert ev0.calls == 2 * k and ev1.calls == 2 * k
    assert ev0.lam == ev1.lam == 0.25 and float(ev1._lam_dev.item()) == 0.25
    h0, h1 = eager.headers().copy(), graphed.headers().copy()
    assert h0["games_done"].min() >= 1
    for f in S.HDR:
        np.testing.assert_array_equal(h0[f], h1[f], err_msg=f)
    x0, x1 = ({key: v.cpu().numpy() for key, v in sp.drain().items()} for sp in (eager, graphed))
    assert len(x0["meta"]) > 0
    # the device queue order is nondeterministic: order both sides by their meta columns
    o0, o1 = np.lexsort(x0["meta"].T[::-1]), np.lexsort(x1["meta"].T[::-1])
    for key in x0:
        np.testing.assert_array_equal(x0[key][o0], x1[key][o1], err_msg=key)
    for sp, ev in ((eager, ev0), (graphed, ev1)):
        assert sp.capacity_events() == NO_EVENTS
        assert ev.unfinished == 0


# ------------------------------------------------------------------ 6. Coach
def test_coach_follows_the_rollout_mix_schedule(tmp_path):
    from splendor import coach as coach_mod
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame
    from splendor.playout import MixedEvaluator
    g = SplendorGame(2)
    nn = NNetWrapper(g, dict(epochs=1, batch_size=256))       # (few training steps: the schedule is the subject)
    seed, B = 4, 8
    args = dict(S.coach_args(tmp_path, rollout_mix=[0.5, 0.25]), numIters=3)
    c = coach_mod.Coach(g, nn, args, batch=B, seed=seed, mem_budget=MEM)
    net_ev, rules = c.sp.evaluator, g.engine.rules
    assert not isinstance(net_ev, MixedEvaluator) and c._mixed_ev == {}
    played, inner = [], c.executeIteration

    def spy(*a, **k):
        ev = c.sp.evaluator
        played.append((ev, getattr(ev, "lam", None), getattr(ev, "calls", None), getattr(ev, "network", None)))
        return inner(*a, **k)
    c.executeIteration = spy
    hist = c.learn()
    assert len(hist) == 3 and len(played) == 3               # learn() completes
    mixed = played[0][0]
    assert isinstance(mixed, MixedEvaluator) and played[1][0] is mixed
    assert [p[1] for p in played] == [0.5, 0.25, None]
    assert type(played[2][0]) is type(net_ev) and played[2][0] is not net_ev
    assert list(c._mixed_ev.values()) == [mixed]             # one instance for the Coach's lifetime
    assert (mixed.playouts, mixed.policy, mixed.seed, mixed.board_base) == (4, "buy_first", seed, 0)
    assert played[0][3] is net_ev and played[1][3] is not net_ev      # refresh_network: the new weights
    calls = [played[0][2], played[1][2], mixed.calls]
    assert calls[0] == 0 < calls[1] < calls[2]               # the counter keeps rising across refresh_network()
    assert mixed.unfinished == 0
    assert type(c.sp.evaluator) is type(net_ev)
    assert len(c.trainExamplesHistory.iters) == 3
    assert g.engine.rules == rules and c.sp.rules == rules
    # one non-zero lambda to another writes the scalar and keeps the graphs; to the network drops them
    assert c.use_mixed_selfplay(0.5) is mixed and c.sp.evaluator is mixed
    c.sp.run(10, use_graph=True)
    g1, gk = c.sp.graph, c.sp.graph_k
    assert g1 is not None and gk is not None
    assert c.use_mixed_selfplay(0.75) is mixed and mixed.lam == 0.75
    assert c.sp.graph is g1 and c.sp.graph_k is gk
    c.sp.run(10, use_graph=True)
    torch.cuda.synchronize()
    assert mixed.calls == calls[2] + 20 and float(mixed._lam_dev.item()) == 0.75
    c.refresh_network()
    assert c.sp.graph is None and c.sp.graph_k is None and type(c.sp.evaluator) is type(net_ev)


# ------------------------------------------------------------------ 7. pit
def pit_records(g, one, two, games=4):
    from splendor.pit import BatchedPit
    pit = BatchedPit(g, one, two, dict(numMCTSSims=8, cpuct=2.5, fpu=0.3), batch=games, seed=5, mem_budget=MEM)
    totals = pit.playGames(games)
    assert sum(totals) == games and pit.capacity == NO_EVENTS
    return totals, pit.last


def same_records(a, b):
    assert a[0] == b[0]
    assert set(a[1]) == set(b[1]) >= {"game", "one_vs_two", "result", "plies", "score", "actions"}
    for k in a[1]:
        np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=k)


def test_mixed_player_in_the_pit():
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame
    from splendor.pit import GreedyPlayer, MCTSPlayer, MixedPlayer
    g = SplendorGame(2)
    net = NNetWrapper(g, dict(dropout=0.0), seed=0)
    runs = [pit_records(g, MixedPlayer(net, 0.5, playouts=2), GreedyPlayer()) for _ in range(2)]
    same_records(*runs)                                      # one seed: the run repeats exactly
    same_records(pit_records(g, MixedPlayer(net, 0.0), MCTSPlayer(net)),
                 pit_records(g, MCTSPlayer(net), MCTSPlayer(net)))
    with pytest.raises(ValueError):
        MixedPlayer(net, 1.5)
