#!/usr/bin/env python3
"""spl_playout launch time against the fused rollout (development tool, GPU).

32,768 mid-game boards (--moves random moves from the deal), one playout per board, both
playout policies. Each playout launch is timed with HIP events and alternates, in one
process, with its comparator: spl_rollout_run on the same boards for K = the longest playout
of that policy, mask_out = NULL (the existing kernel: the same moves plus per-move outputs
and re-deals, every board for all K moves). Median and 10th-90th percentile of --reps
launches after --warmup, the playouts' step-count distribution, and the rates in board-moves
per second (moves actually played for the playout, B K for the rollout).

  python tools/playout_time.py [--players 2] [--boards 32768] [--reps 30] [--out profiles/playout.json]

--mode list: spl_playout_seq on a leaf list against spl_playout(active=) on the same rows: a
fixed seeded --share of the boards (default 0.69, config 3's NN-leaf share) is listed, segment
by segment as spl_mcts_select_compact lists leaves; the two launches alternate in one process
(buy-first playouts, --playouts per leaf), outputs compared bit for bit first.
--mode iteration: ms per self-play iteration (select, playouts, backup, commit) of SelfPlay at
--boards games with the rollout evaluator (--playouts, buy-first) at config 3's search
arguments, eager and as replayed graphs, over --iters iterations after --stagger warm-up
iterations, with the window's capacity events.
--mode mix: spl_playout_mix (lambda 0.5) against spl_playout_seq on the same leaf list, and the
lambda = 0 launch (empty workgroups), alternating in one process; the blend is compared with the
host formula over spl_playout_seq's means first.
--mode mix-iteration: --mode iteration for the network evaluator (seeded random-init network),
the rollout evaluator and the mixed evaluator (lambda 0.5) on three handles in one process.
Every mode prints one JSON record and writes it to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                        # us


def summary(us):
    us = np.asarray(us)
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
            "p90_us": round(float(np.percentile(us, 90)), 1), "launches": int(len(us))}


def listed_leaves(a):
    """The mid-game canonical boards and a seeded --share of them as flags and as the segmented
    leaf list -> (engine, boards, listed, flags, index, count, moves from the deal)."""
    from splendor.env import RolloutBatch, SplendorEngine
    n, B = a.players, a.boards
    e = SplendorEngine(n, device="cuda:0")
    dev = e.device
    rb = RolloutBatch(e, B, seed=a.seed)
    moves = a.moves if a.moves is not None else 20 * n
    rb.run(moves, masks=False)
    st = e.canonical(rb.state, rb.player).contiguous()
    listed = np.random.default_rng(a.seed).random(B) < a.share
    nseg = (B + 63) // 64
    index, count = np.zeros(B, np.int32), np.zeros(nseg, np.int32)
    for j in range(nseg):
        rows = np.flatnonzero(listed[64 * j:64 * j + 64]) + 64 * j
        index[64 * j:64 * j + len(rows)] = rows
        count[j] = len(rows)
    flags = torch.from_numpy(listed.astype(np.uint8)).to(dev)
    return e, st, listed, flags, torch.from_numpy(index).to(dev), torch.from_numpy(count).to(dev), moves


def list_mode(a):
    n, B, P = a.players, a.boards, a.playouts
    e, st, listed, flags, index, count, moves = listed_leaves(a)
    seq = torch.tensor([5], dtype=torch.int32, device=e.device)
    kw = dict(policy="buy_first", playouts=P, seed=a.seed, pi=True)
    o_flag = e.playout(st, active=flags, step0=5 * 256, **kw)
    o_list = e.playout_seq(st, seq, index=index, count=count, **kw)
    o_seqf = e.playout_seq(st, seq, active=flags, **kw)
    torch.cuda.synchronize()
    for o in (o_list, o_seqf):
        assert torch.equal(o["result"], o_flag["result"]) and torch.equal(o["pi"], o_flag["pi"])
    runs = {"playout_flags": lambda: e.playout(st, active=flags, step0=5 * 256, out=o_flag, **kw),
            "playout_seq_list": lambda: e.playout_seq(st, seq, index=index, count=count, out=o_list, **kw),
            "playout_seq_flags": lambda: e.playout_seq(st, seq, active=flags, out=o_seqf, **kw)}
    times = {k: [] for k in runs}
    for rep in range(a.warmup + a.reps):
        for k, fn in runs.items():
            t = timed(fn)
            if rep >= a.warmup:
                times[k].append(t)
    rec = {"mode": "list", "players": n, "boards": B, "playouts": P, "policy": "buy_first", "moves_from_deal": moves,
           "seed": a.seed, "share": a.share, "listed": int(listed.sum()), "outputs_bit_identical": True}
    rec.update({k: summary(v) for k, v in times.items()})
    rec["list_over_flags"] = round(rec["playout_seq_list"]["median_us"] / rec["playout_flags"]["median_us"], 3)
    return rec


def mix_mode(a):
    n, B, P = a.players, a.boards, a.playouts
    e, st, listed, flags, index, count, moves = listed_leaves(a)
    dev = e.device
    seq = torch.tensor([5], dtype=torch.int32, device=dev)
    kw = dict(index=index, count=count, policy="buy_first", playouts=P, seed=a.seed)
    v0 = torch.from_numpy(np.random.default_rng(a.seed).random((B, n), dtype=np.float32) * 2 - 1).to(dev)
    half, zero = (torch.tensor([x], dtype=torch.float32, device=dev) for x in (0.5, 0.0))
    o_seq = e.playout_seq(st, seq, **kw)
    v, unfinished = e.playout_mix(st, seq, half, v0.clone(), **kw)
    vz, _ = e.playout_mix(st, seq, zero, v0.clone(), **kw)
    torch.cuda.synchronize()
    want = np.where(listed[:, None], np.float32(0.5) * v0.cpu().numpy() + np.float32(0.5) * o_seq["result"].cpu().numpy(),
                    v0.cpu().numpy())
    assert np.array_equal(v.cpu().numpy(), want) and torch.equal(vz, v0) and int(unfinished.item()) == 0
    runs = {"playout_seq_list": lambda: e.playout_seq(st, seq, out=o_seq, **kw),
            "playout_mix_list": lambda: e.playout_mix(st, seq, half, v, unfinished=unfinished, **kw),
            "playout_mix_lambda0": lambda: e.playout_mix(st, seq, zero, vz, unfinished=unfinished, **kw)}
    times = {k: [] for k in runs}
    for rep in range(a.warmup + a.reps):
        for k, fn in runs.items():
            t = timed(fn)
            if rep >= a.warmup:
                times[k].append(t)
    rec = {"mode": "mix", "players": n, "boards": B, "playouts": P, "policy": "buy_first", "moves_from_deal": moves,
           "seed": a.seed, "share": a.share, "listed": int(listed.sum()), "blend_equals_host_formula": True}
    rec.update({k: summary(t) for k, t in times.items()})
    s = rec["playout_seq_list"]
    rec["mix_over_seq"] = round(rec["playout_mix_list"]["median_us"] / s["median_us"], 3)
    rec["mix_inside_seq_p10_p90"] = bool(s["p10_us"] <= rec["playout_mix_list"]["median_us"] <= s["p90_us"])
    return rec


def iteration_mode(a, mixed=False):
    from splendor.env import SplendorEngine
    from splendor.playout import MixedEvaluator, PlayoutEvaluator
    from splendor.selfplay import SelfPlay
    n, B, P = a.players, a.boards, a.playouts
    e = SplendorEngine(n, device="cuda:0")
    args = dict(numMCTSSims=100, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5, forced_playouts=False,
                dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
    rec = {"mode": "iteration", "players": n, "games": B, "playouts": P, "policy": "buy_first", "args": args,
           "stagger_iterations": a.stagger, "iterations": a.iters}
    if mixed:
        from splendor.nnet import LeafEvaluator, random_net
        rec["mode"] = "mix-iteration"
        net = random_net(n, seed=0, device="cuda:0")
        for name, make in (("network", lambda: LeafEvaluator(e, net, B, use_graph=False)),
                           ("rollout", lambda: PlayoutEvaluator(e, P, "buy_first", seed=a.seed)),
                           ("mixed", lambda: MixedEvaluator(e, LeafEvaluator(e, net, B, use_graph=False), P,
                                                            "buy_first", lam=0.5, seed=a.seed))):
            sp = SelfPlay(e, B, args, evaluator=make(), dirichlet_noise=True, seed=a.seed,
                          mem_budget=int(0.25 * torch.cuda.mem_get_info()[0]))
            rec[name] = time_iterations(a, sp)
            del sp
        return rec
    sp = SelfPlay(e, B, args, evaluator=PlayoutEvaluator(e, P, "buy_first", seed=a.seed), dirichlet_noise=True,
                  seed=a.seed)
    rec.update(time_iterations(a, sp))
    rec["evaluator_calls"] = sp.evaluator.calls
    return rec


def time_iterations(a, sp):
    """ms per iteration of one handle, graphed then eager, after the warm-up."""
    import time
    rec = {}
    sp.reset()
    sp.run(a.stagger, use_graph=True)
    sp.drain(allow_drops=True)
    for name, graph in (("graphed", True), ("eager", False)):
        torch.cuda.synchronize()
        before = sp.counter_snapshot()
        t0 = time.perf_counter()
        done = 0
        while done < a.iters:                                # (drained as a training run drains)
            sp.run(min(256, a.iters - done), use_graph=graph)
            done += 256
            sp.drain(allow_drops=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d = sp.counter_delta(before, sp.counter_snapshot())
        rec[name] = {"ms_per_iteration": round(dt / a.iters * 1e3, 4), "simulations_per_s": d["sims_backed"] / dt,
                     "moves": d["moves"], "games_done": d["games_done"],
                     "capacity_events": {k: d[k] for k in ("prunes", "resets", "unexpanded")}}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--boards", type=int, default=32768)
    ap.add_argument("--moves", type=int, default=None, help="random moves from the deal (default 20 n)")
    ap.add_argument("--playouts", type=int, default=1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout.json"))
    ap.add_argument("--mode", choices=("launch", "list", "iteration", "mix", "mix-iteration"), default="launch")
    ap.add_argument("--share", type=float, default=0.69, help="list mode: share of the boards that is listed")
    ap.add_argument("--iters", type=int, default=2000, help="iteration mode: timed iterations per variant")
    ap.add_argument("--stagger", type=int, default=600, help="iteration mode: warm-up iterations")
    a = ap.parse_args()
    if a.mode != "launch":
        rec = {"list": list_mode, "iteration": iteration_mode, "mix": mix_mode,
               "mix-iteration": lambda a: iteration_mode(a, mixed=True)}[a.mode](a)
        print(json.dumps(rec, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
    from splendor.env import RolloutBatch, SplendorEngine
    n, B, P = a.players, a.boards, a.playouts
    e = SplendorEngine(n, device="cuda:0")
    dev = e.device
    rb = RolloutBatch(e, B, seed=a.seed)
    moves = a.moves if a.moves is not None else 20 * n
    rb.run(moves, masks=False)
    st, pl = rb.state.clone(), rb.player.clone()
    rec = {"players": n, "boards": B, "playouts": P, "moves_from_deal": moves, "seed": a.seed, "policies": {}}
    runs, dist = {}, {}
    for policy in ("uniform", "buy_first"):
        out = e.playout(st, player=pl, policy=policy, playouts=P, seed=a.seed, steps=True)
        steps = out["steps"].cpu().numpy().ravel()
        assert int(out["unfinished"].item()) == 0
        K = int(steps.max())
        wg = steps.reshape(-1, 64 // P * P).max(1) if steps.size % (64 // P * P) == 0 else steps
        dist[policy] = {"mean": float(steps.mean()), "min": int(steps.min()), "max": K,
                        "percentiles_5_25_50_75_95": [float(x) for x in np.percentile(steps, (5, 25, 50, 75, 95))],
                        "workgroup_longest_mean": float(wg.mean()), "moves_played": int(steps.sum())}
        rs, rp = st.clone(), pl.clone()
        games = torch.zeros(B, dtype=torch.int32, device=dev)
        action = torch.empty((K, B), dtype=torch.int16, device=dev)
        ended = torch.empty((K, B, n), dtype=torch.float32, device=dev)

        def playout(policy=policy, out=out):
            e.playout(st, player=pl, policy=policy, playouts=P, seed=a.seed, steps=True, out=out)

        def restore(rs=rs, rp=rp, games=games):
            rs.copy_(st)
            rp.copy_(pl)
            games.zero_()

        def rollout(K=K, rs=rs, rp=rp, games=games, action=action, ended=ended):
            e.rollout_run(K, rs, rp, None, action, ended, games, a.seed, 0, 0)
        runs[policy] = (playout, restore, rollout, K)
    times = {(p, k): [] for p in runs for k in ("playout", "rollout")}
    for rep in range(a.warmup + a.reps):
        for policy, (playout, restore, rollout, K) in runs.items():
            t = timed(playout)
            restore()
            torch.cuda.synchronize()
            r = timed(rollout)
            if rep >= a.warmup:
                times[policy, "playout"].append(t)
                times[policy, "rollout"].append(r)
    for policy, (_, _, _, K) in runs.items():
        p, r = summary(times[policy, "playout"]), summary(times[policy, "rollout"])
        p["board_moves_per_s"] = dist[policy]["moves_played"] / (p["median_us"] * 1e-6)
        r["K"] = K
        r["board_moves_per_s"] = B * K / (r["median_us"] * 1e-6)
        rec["policies"][policy] = {"steps": dist[policy], "playout": p, "rollout_run": r,
                                   "playout_over_rollout": round(p["median_us"] / r["median_us"], 3)}
    print(json.dumps(rec, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
