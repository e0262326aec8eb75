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
    a = ap.parse_args()
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
