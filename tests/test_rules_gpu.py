"""The reserve-free rules (SplendorGame.disableReserve, SPL_RULE_NO_RESERVE) on the device, bit
for bit: every kernel that builds a legality mask, the search handle, self-play, Coach and the
pit, against the reference run with ENABLE_ACTION_RESERVE = False (tests/golden/noreserve_*,
make_rules_golden.py) and against the rule applied to the full game's masks
(_rules.no_reserve; test_rules.py pins it to the fixtures on the CPU)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _oracle as O  # noqa: E402
import _players as P  # noqa: E402
import _rules as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEM = 1 << 28
NO_EVENTS = {"prunes": 0, "resets": 0, "unexpanded": 0}
RANDOM, GREEDY, POLICY = 0, 1, 2
BUY = np.r_[0:12, 27:30]


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x))                            # (a writable copy: fixtures are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


def engine(n, no_reserve=True):
    """A fresh engine (rules are engine state: tests do not share one)."""
    from splendor.env import SplendorEngine
    e = SplendorEngine(n, device="cuda")
    e.set_rules(no_reserve=no_reserve)
    return e


def masks(e, state, player=None):
    return P.unpack(e.valid_moves(state, player).cpu().numpy())


def in_reserve(actions):
    a = np.asarray(actions)
    return (a >= 12) & (a < 27)


# ------------------------------------------------------------------ 1. spl_valid_moves
@pytest.mark.parametrize("n", (2, 3, 4))
def test_valid_moves_match_reference_and_switch_back(n):
    from splendor.SplendorGame import SplendorGame
    d, full = R.fixture(f"noreserve_env_{n}p.npz"), R.fixture(f"env_{n}p.npz")
    g = SplendorGame(n)
    e = g.engine
    assert g.board.ENABLE_ACTION_RESERVE is True and e.rules == 0
    g.disableReserve()
    assert g.board.ENABLE_ACTION_RESERVE is False and e.rules == R.RULE_NO_RESERVE
    np.testing.assert_array_equal(masks(e, dev(d["canon"])), d["mask_canon"].astype(bool))
    np.testing.assert_array_equal(masks(e, dev(d["state"]), dev(d["player"], torch.int8)),
                                  d["mask_player"].astype(bool))
    np.testing.assert_array_equal(g.getValidMoves(d["canon"][5].copy(), 0), d["mask_canon"][5].astype(bool))
    # the full game's positions under the rule, then the full game again
    np.testing.assert_array_equal(masks(e, dev(full["canon"])), R.no_reserve(full["mask_canon"]))
    g.enableReserve()
    assert g.board.ENABLE_ACTION_RESERVE is True and e.rules == 0
    np.testing.assert_array_equal(masks(e, dev(full["canon"])), full["mask_canon"].astype(bool))
    np.testing.assert_array_equal(masks(e, dev(full["state"]), dev(full["player"], torch.int8)),
                                  full["mask_player"].astype(bool))
    g.board.ENABLE_ACTION_RESERVE = False                        # the reference assigns the attribute
    assert e.rules == R.RULE_NO_RESERVE


@pytest.mark.parametrize("n", (2, 3, 4))
def test_masks_on_arbitrary_byte_boards(n):
    """512 fixture boards with randomly overwritten bytes, half of them with negative bytes (the
    exact-predicate path of the lane-per-board kernels): spl_valid_moves and the fused rollout
    step's mask equal the rule applied to the oracle's mask."""
    d = R.fixture(f"noreserve_env_{n}p.npz")
    rng = np.random.default_rng(31 + n)
    rows = O.rows(n)
    B = 512
    st, pl = d["state"][:B].copy(), d["player"][:B].astype(np.int8)
    hit = np.array([0] + list(range(1, 31)) + list(range(32 + n, rows)))
    for b in range(B):
        for _ in range(rng.integers(1, 6)):
            st[b, rng.choice(hit), rng.integers(0, 7)] = rng.integers(-128 if b % 2 else 0, 12)
    oracle = np.stack([O.valid_moves(n, st[b], int(pl[b])) for b in range(B)])
    want = R.no_reserve(oracle)
    assert (want != oracle.astype(bool)).any(1).sum() > B // 4   # (the rule matters on these boards)
    e = engine(n)
    dst, dpl = dev(st), dev(pl)
    np.testing.assert_array_equal(masks(e, dst, dpl), want)
    mask = torch.zeros((B, 7), dtype=torch.int64, device="cuda")
    act = torch.zeros(B, dtype=torch.int16, device="cuda")
    end = torch.zeros((B, n), dtype=torch.float32, device="cuda")
    games = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.rollout_step(dst, dpl, mask, act, end, games, 0x5EED, 0)
    np.testing.assert_array_equal(P.unpack(mask.cpu().numpy()), want)
    a = act.cpu().numpy()
    assert want[np.arange(B), a].all() and not in_reserve(a).any()


# ------------------------------------------------------------------ 2. spl_player_move
@pytest.mark.parametrize("n", (2, 3, 4))
def test_player_move_candidates_under_the_rule(n):
    d = P.fixture(n)
    e = engine(n)
    B = len(d["board"])
    valid = R.no_reserve(d["valid"])
    after = d["after"].astype(np.int64)
    made_pass = valid[:, R.PASS] & (d["valid"][:, R.PASS] == 0)  # a pass keeps the score
    after[made_pass, R.PASS] = d["s0"][made_pass]
    assert (valid != d["valid"].astype(bool)).any(1).sum() > B // 8 and made_pass.sum() >= 4
    greedy = [P.greedy_candidates(valid[i], int(d["s0"][i]), after[i]) for i in range(B)]
    pi = np.random.default_rng(50 + n).random((B, 409)).astype(np.float32)
    pi[::3, 12:27] = 2.0                                         # the best prior on a reserve move
    want = {RANDOM: (valid, d["s0"]), GREEDY: (np.array([c for c, _ in greedy]), np.array([m for _, m in greedy])),
            POLICY: (np.array([P.policy_candidates(valid[i], pi[i]) for i in range(B)]), d["s0"])}
    st = dev(d["board"])
    seed, stream, base = 0xABCDEF0123456789, 0xFFFFFF, 0xFFFFFF00
    for kind, (cand, best) in want.items():
        action = torch.full((B,), -7, dtype=torch.int16, device="cuda")
        c = torch.full((B, 7), -7, dtype=torch.int64, device="cuda")
        b = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        e.player_move(st, kind, pi=dev(pi) if kind == POLICY else None, seed=seed, stream=stream, board_base=base,
                      out=action, cand_out=c, best_out=b)
        np.testing.assert_array_equal(P.unpack(c.cpu().numpy()), cand, err_msg=f"kind {kind}")
        np.testing.assert_array_equal(b.cpu().numpy(), best, err_msg=f"kind {kind}")
        a = action.cpu().numpy()
        for i in range(B):                                       # the choice keyed as under the full rules
            assert a[i] == P.pick(cand[i], O.uniform(seed, base + i, P.ST_PLAYER | stream, 0)), (kind, i)
        assert not in_reserve(a).any()


# ------------------------------------------------------------------ 3. spl_rollout_run
@pytest.mark.parametrize("n", (2, 4))
def test_rollout_run_is_its_steps_under_the_rule(n):
    """B = 96: one full workgroup and half of one; K = 40 moves in one launch."""
    from splendor.env import RolloutBatch
    B, K, seed = 96, 40, 0x5EED + n
    e = engine(n)
    run = RolloutBatch(e, B, seed=seed)
    out = run.run(K)
    step = RolloutBatch(e, B, seed=seed)
    give = 0
    for k in range(K):
        before = masks(e, step.state, step.player)
        step.step()
        np.testing.assert_array_equal(P.unpack(step.mask.cpu().numpy()), before, err_msg=f"step {k}")
        assert torch.equal(out["mask"][k], step.mask), f"step {k}"
        assert torch.equal(out["action"][k], step.action) and torch.equal(out["ended"][k], step.ended), f"step {k}"
        give += int(before[:, R.RSV_GIVE].any(1).sum())
    for a, b in ((run.state, step.state), (run.player, step.player), (run.games, step.games)):
        assert torch.equal(a, b)
    act = out["action"].cpu().numpy()
    legal = P.unpack(out["mask"].cpu().numpy())
    assert not in_reserve(act).any() and not legal[..., R.RSV].any()
    assert np.take_along_axis(legal, act[..., None].astype(np.int64), 2).all()
    assert give > 0                                              # (reserve + give came up and stayed legal)


# ------------------------------------------------------------------ 4. spl_playout
@functools.lru_cache(maxsize=None)
def playout_start(n, B):
    """Boards after 8 n reserve-free random moves, computed once and left unchanged."""
    from splendor.env import RolloutBatch
    rb = RolloutBatch(engine(n), B, seed=0xC0FFEE)
    rb.run(8 * n, masks=False)
    assert int(rb.games.sum()) == 0
    return rb.state.clone(), rb.player.clone()


@pytest.mark.parametrize("policy", ("uniform", "buy_first"))
@pytest.mark.parametrize("n", (2, 4))
def test_playout_is_the_stepwise_composition(n, policy):
    """B = 40 rows x P = 4 playouts: 16 rows per workgroup, three workgroups, the last partial.
    Against valid_moves / the keyed host pick / step / game_ended, step by step, reserve off."""
    e, B, Pn = engine(n), 40, 4
    seed, step0, base = 77, 40, 0xFFFFFFF0                       # (task ids wrap past 2^32)
    st, pl = playout_start(n, B)
    keep = st.clone()
    out = e.playout(st, player=pl, policy=policy, playouts=Pn, seed=seed, step0=step0, board_base=base, steps=True,
                    pi=True)
    T = B * Pn
    s, p = st.repeat_interleave(Pn, 0).contiguous(), pl.repeat_interleave(Pn, 0).contiguous()
    nxt = torch.empty_like(p)
    outcome, steps = np.zeros((T, n), np.float32), np.zeros(T, np.int32)
    first = None
    for t in range(62 * n):
        valid = masks(e, s, p)
        first = valid if first is None else first
        assert not valid[steps == 0][:, R.RSV].any()
        action, u = np.full(T, R.PASS, np.int16), np.zeros((T, 2))
        for k in np.flatnonzero(steps == 0):
            cand = np.zeros(409, bool)
            if policy == "buy_first":
                cand[BUY] = valid[k][BUY]
            if not cand.any():
                cand = valid[k]
            key = (seed, (base + int(k)) & 0xFFFFFFFF, step0 + t)
            action[k] = P.pick(cand, O.uniform(*key, 0))
            u[k] = O.uniform(*key, 1), O.uniform(*key, 2)
        assert not in_reserve(action).any()
        e.step(s, dev(action), player=p, next_player=nxt, uniforms=dev(u))
        p, nxt = nxt, p
        ended = e.game_ended(s).cpu().numpy()
        new = (ended != 0).any(1) & (steps == 0)
        outcome[new], steps[new] = ended[new], t + 1
        if steps.all():
            break
    assert steps.all() and torch.equal(st, keep)
    np.testing.assert_array_equal(out["steps"].cpu().numpy(), steps.reshape(B, Pn))
    o = outcome.reshape(B, Pn, n)
    mean = np.zeros((B, n), np.float32)
    for j in range(Pn):                                          # f32 sum in ascending j, then / (float)P
        mean = (mean + o[:, j]).astype(np.float32)
    np.testing.assert_array_equal(out["result"].cpu().numpy(), (mean / np.float32(Pn)).astype(np.float32))
    assert int(out["unfinished"].item()) == 0
    v0 = first[::Pn]                                             # the uniform prior is over the rule's mask
    want = np.where(v0, (np.float32(1.0) / v0.sum(1).astype(np.float32))[:, None], np.float32(0))
    np.testing.assert_array_equal(out["pi"].cpu().numpy(), want.astype(np.float32))


# ------------------------------------------------------------------ 5. search
def mcts_for(e, B, sims, cpuct, fpu, forced, **kw):
    from splendor.mcts import BatchedMCTS
    args = dict(numMCTSSims=sims, cpuct=cpuct, fpu=fpu, prob_fullMCTS=1.0, ratio_fullMCTS=5,
                forced_playouts=forced, dirichletAlpha=0.0, temperature=[1.25, 0.8], tempThreshold=10)
    return BatchedMCTS(e, B, args, mem_budget=MEM, **kw)


@pytest.mark.parametrize("n", (2, 4))
def test_searches_match_reference(n):
    """The 18 recorded searches on handles created with rules=, on an engine that plays the full
    game before and after; then the 30-move kept-tree game on a handle that takes a
    reserve-free engine's rules."""
    d = R.fixture(f"noreserve_mcts_{n}p.npz")
    e = engine(n, no_reserve=False)
    for c in sorted(set(int(c) for c in d["case"])):
        idx = np.flatnonzero(d["case"] == c)
        i0 = idx[0]
        m = mcts_for(e, len(idx), int(d["sims"][i0]), float(d["cpuct"][i0]), float(d["fpu"][i0]),
                     bool(d["forced"][i0]), rules=R.RULE_NO_RESERVE)
        assert m.rules == R.RULE_NO_RESERVE and e.rules == 0
        probs, q, _, counts = m.get_action_prob(dev(d["root"][idx]), force_full_search=True, keep_tree=False)
        _, qsa, _, _ = m.root_stats()
        np.testing.assert_array_equal(counts.cpu().numpy(), d["counts"][idx], err_msg=f"case {c}")
        np.testing.assert_array_equal(qsa.cpu().numpy(), d["qsa"][idx])
        np.testing.assert_array_equal(probs.cpu().numpy(), d["probs"][idx])
        np.testing.assert_array_equal(q.cpu().numpy(), d["q"][idx])
        assert m.capacity_events() == NO_EVENTS
    e.set_rules(no_reserve=True)
    m = mcts_for(e, 1, 50, 2.5, 0.3, False)
    e.set_rules(no_reserve=False)                                # the handle keeps what it was created under
    assert m.rules == R.RULE_NO_RESERVE and e.rules == 0
    for k in range(len(d["seq_root"])):
        probs, q, _, counts = m.get_action_prob(dev(d["seq_root"][k][None]), force_full_search=True, keep_tree=True)
        np.testing.assert_array_equal(counts.cpu().numpy()[0], d["seq_counts"][k], err_msg=f"move {k}")
        np.testing.assert_array_equal(probs.cpu().numpy()[0], d["seq_probs"][k])
        np.testing.assert_array_equal(q.cpu().numpy()[0], d["seq_q"][k])
    assert m.capacity_events() == NO_EVENTS
    full = mcts_for(e, 1, 50, 2.5, 0.3, False)                   # and a full-rules handle beside it
    assert full.rules == 0
    counts = full.get_action_prob(dev(d["seq_root"][0][None]), keep_tree=False)[3].cpu().numpy()
    assert counts[0, R.RSV].any()


# ------------------------------------------------------------------ 6. self-play
@pytest.mark.parametrize("tag", ("2p", "4p"))
def test_episode_matches_reference(tag):
    """A whole reserve-free reference episode (root noise, temperature sampling, chance,
    symmetries) replayed on a reserve-free self-play handle with graph replay: the reference's
    example list, bit for bit."""
    from splendor.coach import expand_symmetries
    from splendor.env import unpack_mask
    from splendor.selfplay import SelfPlay
    d = R.fixture(f"noreserve_episode_{tag}.npz")
    n = {56: 2, 88: 4}[d["board"].shape[1]]
    a = {k[4:]: d[k] for k in d if k.startswith("arg_")}
    args = dict(numMCTSSims=int(a["numMCTSSims"]), cpuct=float(a["cpuct"]), fpu=float(a["fpu"]),
                prob_fullMCTS=float(a["prob_fullMCTS"]), ratio_fullMCTS=int(a["ratio_fullMCTS"]),
                forced_playouts=bool(a["forced_playouts"]), dirichletAlpha=float(a["dirichletAlpha"]),
                temperature=[float(x) for x in a["temperature"]], tempThreshold=int(a["tempThreshold"]))
    e = engine(n, no_reserve=False)
    (gb,) = d["game_board_id"]
    sp = SelfPlay(e, 1, args, dirichlet_noise=True, seed=int(d["seed"]), board_base=int(gb), out_cap=4096,
                  mem_budget=MEM, rules=R.RULE_NO_RESERVE)
    assert sp.rules == R.RULE_NO_RESERVE and e.rules == 0
    sp.reset()
    runs = 0
    while sp.stats()["games_done"] == 0:
        sp.run(256, use_graph=True)
        runs += 1
        assert runs < 64, "episode did not finish"
    assert sp.capacity_events() == NO_EVENTS
    ex = sp.drain()
    keep = ex["meta"][:, 1] == 0
    ex = {k: v[keep] for k, v in ex.items()}
    order = torch.argsort(ex["meta"][:, 2])
    ex = expand_symmetries(e, {k: v[order] for k, v in ex.items()})
    assert ex["board"].shape[0] == len(d["board"]) == int(d["game_n_examples"][0])
    np.testing.assert_array_equal(ex["board"].cpu().numpy(), d["board"])
    np.testing.assert_array_equal(ex["pi"].cpu().numpy(), d["pi"])
    np.testing.assert_array_equal(unpack_mask(ex["valids"]).cpu().numpy().astype(np.uint8), d["valids"])
    np.testing.assert_array_equal(ex["winner"].cpu().numpy(), d["winner"])
    np.testing.assert_array_equal(ex["scdiff"].cpu().numpy(), d["scdiff"])
    np.testing.assert_array_equal(ex["surprise"].cpu().numpy(), d["surprise"].astype(np.float32))


# ------------------------------------------------------------------ 7. Coach and the pit
def test_coach_trains_without_and_validates_with(tmp_path):
    from splendor.SplendorGame import SplendorGame
    from splendor.coach import Coach
    from splendor.mcts import HashEvaluator
    from splendor.pit import BatchedPit, GreedyPlayer, RandomPlayer
    args = dict(numMCTSSims=8, cpuct=1.5, fpu=0.1, prob_fullMCTS=1.0, ratio_fullMCTS=4, forced_playouts=False,
                dirichletAlpha=0.0, temperature=[1.25, 0.8], tempThreshold=10, numItersHistory=3,
                checkpoint=str(tmp_path), selfplay_reserve=False)
    g = SplendorGame(2)
    e = g.engine
    c = Coach(g, None, args, batch=32, seed=5, mem_budget=MEM)
    c.sp.evaluator = HashEvaluator(e)
    assert c.sp.rules == R.RULE_NO_RESERVE and e.rules == 0
    ex = c.executeEpisodes(32, as_tuples=False)
    assert ex["board"].shape[0] > 32 * 10
    valids, pi = P.unpack(ex["valids"].cpu().numpy()), ex["pi"].cpu().numpy()
    assert not valids[:, R.RSV].any() and not pi[:, R.RSV].any()
    assert not pi[~valids].any()
    assert e.rules == 0 and g.board.ENABLE_ACTION_RESERVE is True
    deal = e.init(e.new_state(4), seed=1)
    assert masks(e, deal)[:, R.RSV].all()                        # a fresh deal: every reserve is legal
    default = Coach(g, None, dict(args, selfplay_reserve=True), batch=4, seed=5, mem_budget=MEM)
    assert default.sp.rules == 0
    # validate with: the pit under the full rules in the same process
    pit = BatchedPit(g, GreedyPlayer(), RandomPlayer(), batch=64, seed=3)
    assert sum(pit.playGames(64)) == 64
    assert in_reserve(pit.last["actions"]).any()
    # and under tools/pit.py --no-reserve's semantics
    g.disableReserve()
    pit = BatchedPit(g, GreedyPlayer(), RandomPlayer(), batch=64, seed=3)
    one, two, draws = pit.playGames(64)
    assert one + two + draws == 64 and (pit.last["plies"] > 0).all()
    assert not in_reserve(pit.last["actions"]).any()
    assert ((pit.last["actions"] >= 290) & (pit.last["actions"] < 365)).any()
    g.enableReserve()
