#!/usr/bin/env python3
"""Stored size and batch-assembly time of the two forms of the example store, one process,
2 players:
  * one example set from seeded self-play (Coach.executeEpisodes on GAMES concurrent games
    until FINISH have ended, genbu search arguments at SIMS simulations, seeded random-init
    network), kept unexpanded; the materialised form is expand_symmetries of the same rows;
  * stored bytes of both forms and the mean number of variants per position;
  * the time to assemble one training batch for the same row ids on both paths, at batch
    sizes 32 and 4096: "materialised" is the five index_selects + int8->f32 cast +
    unpack_mask that NNetWrapper.train runs on an ExampleSet, "lazy" is
    LazySymmetryExamples.batch(ids) (searchsorted + one gather kernel). Per batch size the two
    paths alternate, WARM untimed rounds then REPS timed ones on fresh ids each round; a
    sample is a host clock around the call, closed by a device synchronise. Median, 10th /
    90th percentile and extremes are reported; nothing is asserted.
Writes one JSON object to --out (default profiles/lazy_symmetries.json) and prints it:
    python3 tools/example_batch_time.py [--games G] [--finish F] [--sims S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))

from splendor.NNet import NNetWrapper  # noqa: E402
from splendor.SplendorGame import SplendorGame  # noqa: E402
from splendor.coach import Coach, expand_symmetries  # noqa: E402
from splendor.env import unpack_mask  # noqa: E402
from splendor.examples import FIELDS, ExampleSet, LazySymmetryExamples  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096, help="concurrent self-play games")
ap.add_argument("--finish", type=int, default=2048, help="games to finish before the examples are taken")
ap.add_argument("--sims", type=int, default=25)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lazy_symmetries.json"))
a = ap.parse_args()

N, WARM, REPS, BATCHES, SEED = 2, 20, 200, (32, 4096), 0x5EED
ARGS = dict(numMCTSSims=a.sims, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5,
            forced_playouts=False, dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)

torch.manual_seed(0)
game = SplendorGame(N)
dev = game.engine.device
coach = Coach(game, NNetWrapper(game, seed=0), ARGS, batch=a.games, seed=SEED)
t0 = time.perf_counter()
ex = coach.executeEpisodes(a.finish, with_symmetries=False, as_tuples=False)
torch.cuda.synchronize(dev)
selfplay_s = time.perf_counter() - t0
del coach
lazy = LazySymmetryExamples(ExampleSet.from_drain(ex), game.engine)
mat = ExampleSet.from_drain(expand_symmetries(game.engine, {k: ex[k] for k in FIELDS}))
torch.cuda.synchronize(dev)
assert len(mat) == len(lazy)


def nbytes(s):
    return sum(getattr(s, k).numel() * getattr(s, k).element_size() for k in FIELDS)


def materialised_batch(ids):          # NNetWrapper.train's assembly for an ExampleSet
    boards = mat.board.index_select(0, ids).float()
    valids = unpack_mask(mat.valids.index_select(0, ids))
    return boards, mat.pi.index_select(0, ids), mat.winner.index_select(0, ids), \
        mat.scdiff.index_select(0, ids), valids


def timed(fn, ids):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn(ids)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e6, out


def summary(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)),
            "p90_us": float(np.percentile(us, 90)), "min_us": float(us.min()), "max_us": float(us.max())}


lazy_stored = nbytes(lazy.base) + lazy.counts.numel() + 8 * lazy.offsets.numel()
out = {"players": N, "device": torch.cuda.get_device_name(dev),
       "examples": {"source": "seeded self-play", "concurrent_games": a.games, "games_finished_at_least": a.finish,
                    "simulations": a.sims, "selfplay_seconds": selfplay_s, "positions": lazy.n_base,
                    "variants": len(lazy), "mean_variants_per_position": len(lazy) / lazy.n_base},
       "stored_bytes": {"materialised": nbytes(mat), "lazy": lazy_stored,
                        "lazy_counts_and_offsets": lazy.counts.numel() + 8 * lazy.offsets.numel(),
                        "ratio": nbytes(mat) / lazy_stored},
       "timing": {"clock": "host perf_counter around the call, device synchronise before and after",
                  "warmup_rounds": WARM, "timed_rounds": REPS, "order": "materialised, lazy alternating per round"},
       "batch_assembly": {}}

gen = torch.Generator(device=dev)
gen.manual_seed(1)
for bs in BATCHES:
    if bs > len(lazy):
        continue
    us = {"materialised": [], "lazy": []}
    for r in range(WARM + REPS):
        ids = torch.randperm(len(lazy), generator=gen, device=dev)[:bs]
        tm, om = timed(materialised_batch, ids)
        tl, ol = timed(lazy.batch, ids)
        if r == 0:                     # the two paths give the same tensors
            assert all(torch.equal(x, y) for x, y in zip(om, ol))
        if r >= WARM:
            us["materialised"].append(tm)
            us["lazy"].append(tl)
    lazy.check_errors()
    res = {k: summary(v) for k, v in us.items()}
    res["lazy_over_materialised_median"] = res["lazy"]["median_us"] / res["materialised"]["median_us"]
    out["batch_assembly"][str(bs)] = res

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
