#!/usr/bin/env python3
"""The two figures of profiles/review.json, one run each, reported as found (no threshold):

* the spl_mcts_pv launch (lines=3, depth=8) against the spl_mcts_root_stats launch, in the same
  run, on 32,768 trees after a BASELINE config-3 search (2 players, 100 simulations, cpuct 2.5,
  fpu 0.3) from midgame roots under the hash network (mode 1: peaked priors, deep trees);
* reviewed positions per second at 100 and 1,600 simulations for a 64-game record (greedy
  against random), the reviewer a rollout player (buy_first, one playout per leaf), wall time
  of splendor.review.review() including the replay and the handle's creation.

    python3 tools/review_profile.py --out profiles/review.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))


def launch_times(fns, reps, burst=20):
    """Device-event time per launch of each of `fns` (name -> launch into preallocated
    outputs), `burst` back-to-back launches per event pair, the kernels alternating."""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(burst):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / burst)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "bursts": reps,
                "launches_per_burst": burst} for k, v in us.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "review.json"))
    ap.add_argument("--trees", type=int, default=32768)
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, nargs="+", default=[100, 1600])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    from splendor.SplendorGame import SplendorGame
    from splendor.env import RolloutBatch
    from splendor.mcts import BatchedMCTS, HashEvaluator
    from splendor.pit import BatchedPit, GreedyPlayer, RandomPlayer
    from splendor.playout import PlayoutEvaluator
    from splendor.review import review
    out = {"device": torch.cuda.get_device_name(0)}
    game = SplendorGame(2)
    e = game.engine

    # ---- the walk against root_stats
    B = a.trees
    rb = RolloutBatch(e, B, seed=0x5EED)
    for _ in range(20):
        rb.step()
    roots = e.canonical(rb.state, rb.player)
    args = dict(numMCTSSims=100, cpuct=2.5, fpu=0.3, prob_fullMCTS=1.0, ratio_fullMCTS=5, forced_playouts=False,
                dirichletAlpha=0.0, temperature=[1.25, 0.8], tempThreshold=10)
    m = BatchedMCTS(e, B, args, evaluator=HashEvaluator(e, mode=1))
    m.get_action_prob(roots, keep_tree=False)
    pv = m.principal_variations(3, 8)
    ln = pv["length"].cpu().numpy()
    hdr = m.headers()
    rs = m.root_stats()
    s, p = e._s(), lambda t: C.c_void_p(t.data_ptr())
    times = launch_times({
        "k_pv": lambda: m.L.spl_mcts_pv(m.h, 3, 8, p(pv["action"]), p(pv["visits"]), p(pv["q"]), p(pv["prior"]),
                                        p(pv["length"]), p(pv["end"]), s),
        "k_root_stats": lambda: m.L.spl_mcts_root_stats(m.h, p(rs[0]), p(rs[1]), p(rs[2]), p(rs[3]), None, s)},
        a.reps)
    out["pv_launch"] = {
        "trees": B, "lines": 3, "depth": 8, "search": "config 3 (2 players, 100 simulations), hash network mode 1",
        **times,
        "note": "device events around bursts of launches into preallocated outputs; root_stats writes 3 x 409 "
                "8-byte entries per tree (counts, qsa, probs) and q, pv 4 x 24 entries + 2 x 3",
        "mean_line_length": float(ln[ln > 0].mean()), "max_line_length": int(ln.max()),
        "end_codes": np.bincount(pv["end"].cpu().numpy().ravel(), minlength=5).tolist(),
        "mean_leaf_depth": float(hdr["depth_sum"].sum() / max(int(hdr["sims_backed"].sum()), 1))}
    del m, pv
    torch.cuda.empty_cache()
    print(json.dumps(out["pv_launch"]), flush=True)

    # ---- positions per second
    pit = BatchedPit(game, GreedyPlayer(), RandomPlayer(), batch=a.games, seed=0x5EED)
    pit.playGames(a.games)
    rec = pit.record()
    out["review"] = []
    for sims in a.sims:
        margs = dict(numMCTSSims=sims, cpuct=2.5, fpu=0.3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = review(game, PlayoutEvaluator(e, playouts=1), rec, margs, lines=3, depth=8)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        N = len(r["ply"])
        row = {"games": a.games, "positions": N, "numMCTSSims": sims, "reviewer": "rollout:buy_first:1",
               "seconds": s, "positions_per_second": N / s, "mean_entropy": float(r["entropy"].mean()),
               "mean_q_loss": float(np.nanmean(r["q_loss"])), "played_is_best": float((r["played_rank"] == 0).mean()),
               "mean_line0_length": float(r["pv_length"][:, 0].mean())}
        out["review"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
