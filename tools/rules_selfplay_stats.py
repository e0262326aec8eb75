#!/usr/bin/env python3
"""Plies per game and mean legal moves of self-play at config 3's search arguments (genbu.pt's:
100 simulations, cpuct 2.5, fpu 0.3, 25 % full searches, root noise; seeded random-init
SplendorNNet), 4,096 concurrent games, under the full rules and reserve-free: each tree's first
game, legal moves counted on the recorded (full-search) positions. One JSON line per rule set;
    python3 tools/rules_selfplay_stats.py [games] [OUT.json]
profiles/no_reserve.json holds a run."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))
from splendor.env import SplendorEngine, unpack_mask  # noqa: E402
from splendor.nnet import LeafEvaluator, random_net  # noqa: E402
from splendor.selfplay import SelfPlay  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ARGS = dict(numMCTSSims=100, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5, forced_playouts=False,
            dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
out = []
for rules in (0, 1):
    e = SplendorEngine(2)
    sp = SelfPlay(e, B, ARGS, evaluator=LeafEvaluator(e, random_net(2, seed=0), B), dirichlet_noise=True,
                  seed=0x5EED, mem_budget=32 << 30, rules=rules)
    sp.reset()
    first = np.full(B, -1, np.int64)
    legal, rsv_give, npos, iters = 0, 0, 0, 0
    t0 = time.perf_counter()
    while (first < 0).any() and iters < 40000:
        sp.run(64, use_graph=True)
        iters += 64
        h = sp.headers()
        new = (first < 0) & (h["games_done"] == 1)
        first[new] = h["moves"][new] - h["episode_step"][new]
        late = (first < 0) & (h["games_done"] > 1)                 # (two games ended inside one chunk)
        first[late] = 0
        ex = sp.drain()
        if ex["valids"].shape[0]:
            v = unpack_mask(ex["valids"])
            legal += int(v.sum())
            rsv_give += int(v[:, 290:365].any(1).sum())
            npos += v.shape[0]
    torch.cuda.synchronize()
    st = sp.stats()
    ok = first > 0
    rec = {"rules": rules, "games": B, "iterations": iters, "seconds": time.perf_counter() - t0,
           "first_games_counted": int(ok.sum()), "plies_per_game_mean": float(first[ok].mean()),
           "plies_per_game_max": int(first[ok].max()), "recorded_positions": npos,
           "legal_moves_mean": legal / max(npos, 1), "positions_with_reserve_and_give": rsv_give,
           "capacity_events": sp.capacity_events(), "overflow": st["overflow"]}
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del sp
    torch.cuda.empty_cache()
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
