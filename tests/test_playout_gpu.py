"""spl_playout on the device, bit for bit: uniform playouts against the existing fused rollout
(the same moves from the same Philox streams), buy-first playouts against a stepwise
composition of valid_moves / the keyed host pick / step / game_ended, truncation by
max_steps, and the evaluator inside the search and the pit.

Workgroup geometry of k_playout: 64 / P rows (their (64 / P) P tasks) per workgroup, so with
B = 70 rows, P = 1 gives one full and one partial workgroup (6 tasks) and P = 3 gives 21 rows
= 63 tasks per workgroup (one idle lane) over 4 workgroups, the last with 7 rows; task ids
b P + j run across the workgroup boundaries."""
import functools
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _players as P  # noqa: E402

sys.path.insert(0, P.GOLD)
import detrand  # noqa: E402

pytestmark = pytest.mark.gpu

MEM = 1 << 28
BUY = np.r_[0:12, 27:30]


@functools.lru_cache(maxsize=None)
def engine(n):
    from splendor.env import SplendorEngine
    return SplendorEngine(n, device="cuda")


def midgame(n, B, moves, seed=0xC0FFEE):
    """(state int8 [B,R,7], player int8 [B]) after `moves` random moves from the deal."""
    from splendor.env import RolloutBatch
    rb = RolloutBatch(engine(n), B, seed=seed)
    rb.run(moves, masks=False)
    assert int(rb.games.sum()) == 0                          # (no game is over: nothing re-dealt)
    return rb.state.clone(), rb.player.clone()


def seq_mean(o):
    """f32 sum of o[..., j, :] in ascending j, then / (float)P, as the header defines."""
    s = np.zeros(o.shape[:-2] + o.shape[-1:], np.float32)
    for j in range(o.shape[-2]):
        s = (s + o[..., j, :]).astype(np.float32)
    return (s / np.float32(o.shape[-2])).astype(np.float32)


SEED, STEP0, BASE = 0x1234ABCD5EED, 1000, 0xFFFFFFC0        # (board ids wrap past 2^32)


@functools.lru_cache(maxsize=None)
def rollout_reference(n, B, Pn):
    """Every row replicated Pn times (task order) through spl_rollout_run for 62 n moves ->
    (state, player, outcome [B,Pn,n], steps [B,Pn]): a task's outcome is its first non-zero
    end vector. Computed once per shape and left unchanged."""
    e = engine(n)
    st, pl = midgame(n, B, 20 * n)
    T, K, dev = B * Pn, 62 * n, e.device
    rs, rp = st.repeat_interleave(Pn, 0).contiguous(), pl.repeat_interleave(Pn, 0).contiguous()
    action = torch.empty((K, T), dtype=torch.int16, device=dev)
    ended = torch.empty((K, T, n), dtype=torch.float32, device=dev)
    games = torch.zeros(T, dtype=torch.int32, device=dev)
    e.rollout_run(K, rs, rp, None, action, ended, games, SEED, STEP0, BASE)
    ended = ended.cpu().numpy()
    over = (ended != 0).any(2)                               # [K, T]
    assert over.any(0).all()
    first = over.argmax(0)
    outcome = ended[first, np.arange(T)].reshape(B, Pn, n)
    steps = (first + 1).astype(np.int32).reshape(B, Pn)
    for a in (outcome, steps):
        a.setflags(write=False)
    return st, pl, outcome, steps


@pytest.mark.parametrize("Pn", (1, 3))
@pytest.mark.parametrize("n", (2, 3, 4))
def test_uniform_playouts_are_the_rollout(n, Pn):
    e, B = engine(n), 70
    st, pl, outcome, steps = rollout_reference(n, B, Pn)
    assert steps.max() - steps.min() > 10                    # (game lengths differ widely)
    active = (np.arange(B) % 5 != 2).astype(np.uint8)
    dev = e.device
    out = {"result": torch.full((B, n), -7.0, dtype=torch.float32, device=dev),
           "pi": torch.full((B, 409), -7.0, dtype=torch.float32, device=dev),
           "steps": torch.full((B, Pn), -7, dtype=torch.int32, device=dev)}
    keep = st.clone()
    out = e.playout(st, player=pl, active=torch.from_numpy(active).to(dev), policy="uniform", playouts=Pn,
                    max_steps=62 * n, seed=SEED, step0=STEP0, board_base=BASE, pi=True, steps=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(st, keep)                             # the input boards are read only
    on, off = active != 0, active == 0
    res, pi, ns = (out[k].cpu().numpy() for k in ("result", "pi", "steps"))
    np.testing.assert_array_equal(ns[on], steps[on])
    np.testing.assert_array_equal(res[on], seq_mean(outcome)[on])
    assert int(out["unfinished"].item()) == 0
    assert (res[off] == -7).all() and (pi[off] == -7).all() and (ns[off] == -7).all()
    valid = P.unpack(e.valid_moves(st, pl).cpu().numpy())
    want = np.where(valid, (np.float32(1.0) / valid.sum(1).astype(np.float32))[:, None], np.float32(0))
    np.testing.assert_array_equal(pi[on], want.astype(np.float32)[on])


@pytest.mark.parametrize("Pn", (33, 64))
def test_one_row_per_workgroup(Pn):
    """P > 32: a workgroup holds one row (31 idle lanes at P = 33, none at P = 64); the f32 sum
    runs over many outcomes in task order."""
    n, B = 2, 3
    e = engine(n)
    st, pl, outcome, steps = rollout_reference(n, B, Pn)
    out = e.playout(st, player=pl, policy="uniform", playouts=Pn, seed=SEED, step0=STEP0, board_base=BASE,
                    steps=True)
    np.testing.assert_array_equal(out["steps"].cpu().numpy(), steps)
    np.testing.assert_array_equal(out["result"].cpu().numpy(), seq_mean(outcome))
    assert int(out["unfinished"].item()) == 0


def test_uniform_playouts_without_optional_arguments():
    """NULL player / active / pi_out / steps_out / unfinished: canonical leaves, result only."""
    from splendor import _lib
    from splendor.env import _ptr
    n, B, Pn = 2, 70, 3
    e = engine(n)
    st, pl, outcome, _ = rollout_reference(n, B, Pn)
    canon = e.canonical(st, pl)                              # mover = seat 0: outcomes rolled by -player
    res = torch.empty((B, n), dtype=torch.float32, device=e.device)
    _lib.check(e.L.spl_playout(e.ctx, B, _ptr(canon), None, None, _lib.PLAYOUT_UNIFORM, Pn, 62 * n, SEED, STEP0,
                               BASE, _ptr(res), None, None, None, e._s()), "spl_playout")
    p = pl.cpu().numpy()
    want = np.stack([np.roll(outcome[b], -int(p[b]), axis=-1) for b in range(B)])
    np.testing.assert_array_equal(res.cpu().numpy(), seq_mean(want))


@pytest.mark.parametrize("n", (2, 4))
def test_buy_first_is_the_stepwise_composition(n):
    e, B, Pn = engine(n), 16, 2
    seed, step0, base = 77, 40, 9
    st, pl = midgame(n, B, 8 * n, seed=5)
    out = e.playout(st, player=pl, policy="buy_first", playouts=Pn, seed=seed, step0=step0, board_base=base,
                    steps=True)
    T, dev = B * Pn, e.device
    s, p = st.repeat_interleave(Pn, 0).contiguous(), pl.repeat_interleave(Pn, 0).contiguous()
    nxt = torch.empty_like(p)
    outcome, steps = np.zeros((T, n), np.float32), np.zeros(T, np.int32)
    bought = 0
    for t in range(62 * n):
        valid = P.unpack(e.valid_moves(s, p).cpu().numpy())
        action, u = np.zeros(T, np.int16), np.zeros((T, 2))
        for k in range(T):
            cand = np.zeros(409, bool)
            cand[BUY] = valid[k][BUY]
            bought += int(cand.any() and not steps[k])
            if not cand.any():
                cand = valid[k]
            key = (seed, base + k, step0 + t)
            action[k] = P.pick(cand, detrand.uniform(*key, 0))
            u[k] = detrand.uniform(*key, 1), detrand.uniform(*key, 2)
        e.step(s, torch.from_numpy(action).to(dev), player=p, next_player=nxt,
               uniforms=torch.from_numpy(u).to(dev))
        p, nxt = nxt, p
        ended = e.game_ended(s).cpu().numpy()
        new = (ended != 0).any(1) & (steps == 0)
        outcome[new], steps[new] = ended[new], t + 1
        if steps.all():
            break
    assert steps.all() and bought > T                        # (the buy branch was taken)
    np.testing.assert_array_equal(out["steps"].cpu().numpy(), steps.reshape(B, Pn))
    np.testing.assert_array_equal(out["result"].cpu().numpy(), seq_mean(outcome.reshape(B, Pn, n)))
    assert int(out["unfinished"].item()) == 0


@pytest.mark.parametrize("policy", ("uniform", "buy_first"))
def test_truncation(policy):
    """No game can end in 5 moves from the deal: zero results, 5 steps, every task unfinished."""
    n, B, Pn = 3, 37, 4
    e = engine(n)
    st = e.init(e.new_state(B), seed=3)
    out = e.playout(st, policy=policy, playouts=Pn, max_steps=5, seed=11, steps=True)
    out["result"].fill_(-7.0)
    out = e.playout(st, policy=policy, playouts=Pn, max_steps=5, seed=11, steps=True, out=out)
    assert (out["result"].cpu().numpy() == 0).all()
    assert (out["steps"].cpu().numpy() == 5).all()
    assert int(out["unfinished"].item()) == 2 * B * Pn          # (the reused counter adds up)


def searched(n, B, sims, seed, playouts):
    from splendor.mcts import BatchedMCTS
    from splendor.playout import PlayoutEvaluator
    e = engine(n)
    ev = PlayoutEvaluator(e, playouts=playouts, policy="buy_first", seed=seed, board_base=3)
    seen = []

    def spy(state, mask, valid):
        pi, v = ev(state, mask, valid)
        if not seen:
            seen.append((state.clone(), mask.clone(), valid.clone(), pi.clone(), v.clone()))
        return pi, v
    m = BatchedMCTS(e, B, dict(numMCTSSims=sims, cpuct=2.5, fpu=0.3), evaluator=spy, seed=seed, mem_budget=MEM)
    roots = e.init(e.new_state(B), seed=seed)
    counts = m.get_action_prob(roots)[3].cpu().numpy()
    return e, m, ev, seen[0], counts


def test_evaluator_in_the_search():
    n, B, sims, seed, Pn = 2, 8, 16, 21, 2
    e, m, ev, (state, mask, valid, pi, v), counts = searched(n, B, sims, seed, Pn)
    assert ev.calls == sims and bool(valid.all())
    direct = e.playout(state, active=valid, policy="buy_first", playouts=Pn, seed=seed, step0=0, board_base=3,
                       pi=True)
    assert torch.equal(direct["result"], v) and torch.equal(direct["pi"], pi)
    legal = P.unpack(mask.cpu().numpy())
    np.testing.assert_array_equal(pi.cpu().numpy() > 0, legal)
    assert (np.abs(v.cpu().numpy()) <= 1).all()
    # the simulation that creates the root visits no edge: sims - 1 root visits
    assert (counts.sum(1) == sims - 1).all()
    assert m.capacity_events() == {"prunes": 0, "resets": 0, "unexpanded": 0}
    again = searched(n, B, sims, seed, Pn)[4]
    np.testing.assert_array_equal(again, counts)
    assert (searched(n, B, sims, seed + 1, Pn)[4] != counts).any()


def assert_end_vectors(r):
    """check_end's outcomes: one winner (+1, the others -1) or a shared win (0.01 each, >= 2)."""
    r = np.asarray(r, np.float32)
    win, share, lose = r == 1.0, r == np.float32(0.01), r == -1.0
    assert (win | share | lose).all()
    assert (((win.sum(1) == 1) & (share.sum(1) == 0)) | ((win.sum(1) == 0) & (share.sum(1) >= 2))).all()


def test_pit_seats_rollout_players():
    from splendor.SplendorGame import SplendorGame
    from splendor.pit import BatchedPit, RandomPlayer, RolloutPlayer
    g = SplendorGame(2)
    runs = []
    for _ in range(2):
        pit = BatchedPit(g, RolloutPlayer(numMCTSSims=8), RandomPlayer(), dict(cpuct=2.5, fpu=0.3), batch=8, seed=9,
                         mem_budget=MEM)
        assert len(pit.mcts) == 1 and pit.mcts[0].cfg.num_sims == 8
        totals = pit.playGames(8)
        assert sum(totals) == 8
        assert_end_vectors(pit.last["result"])
        assert (pit.last["plies"] > 0).all()
        assert pit.capacity == {"prunes": 0, "resets": 0, "unexpanded": 0}
        runs.append((totals, pit.last))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k], err_msg=k)


def test_pit_seats_two_rollout_players(monkeypatch):
    """Two RolloutPlayers together: two trees, no network and no network evaluator."""
    from splendor import pit
    from splendor.SplendorGame import SplendorGame

    def no_net(*a, **k):
        raise AssertionError("a network evaluator was built for a rollout player")
    monkeypatch.setattr(pit, "evaluator_for", no_net)
    g = SplendorGame(2)
    p = pit.BatchedPit(g, pit.RolloutPlayer(numMCTSSims=4, playouts=2), pit.RolloutPlayer(numMCTSSims=6,
                       policy="uniform"), batch=4, seed=2, mem_budget=MEM)
    assert [m.cfg.num_sims for m in p.mcts] == [4, 6]
    evs = [m.evaluator for m in p.mcts]
    assert [(ev.playouts, ev.policy) for ev in evs] == [(2, "buy_first"), (1, "uniform")]
    assert evs[0].seed != evs[1].seed
    assert sum(p.playGames(4)) == 4
    assert all(ev.calls > 0 for ev in evs)
    assert_end_vectors(p.last["result"])
