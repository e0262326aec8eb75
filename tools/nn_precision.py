#!/usr/bin/env python3
"""The fused network kernel's precision modes ("f32", "bf16x2", "bf16": spl_nn_forward_mode)
measured side by side in one process, 2 players:
  * full batch: B leaf boards (fresh deals + 30 random plies each: every game stage), WARM
    untimed launches, then ITERS launches per mode timed with HIP events on the launch stream;
  * error: max |pi - pi64| and |v - v64| per mode against FoldedNet in float64, for the seeded
    random-init network and, when the file exists, a tools/train_prior.py checkpoint;
  * self-play: per mode a SelfPlay of config 3's shape (genbu arguments, 100 simulations) over
    GAMES games, PREFILL untimed iterations then STEPS timed ones (early-game trees: no phase
    stagger, so the figures compare the modes with one another, not with the headline);
  * --arena: one network against itself, "bf16" (player 1) vs "f32" (player 2), BatchedArena,
    100 simulations, 256 games (a record, not a test).
Prints one JSON object (and writes it to --out):
    python3 tools/nn_precision.py [--leaves B] [--games G] [--net CKPT.pt] [--arena] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))

from splendor.env import RolloutBatch, SplendorEngine  # noqa: E402
from splendor.nnet import PRECISIONS, FoldedNet, LeafEvaluator, random_net  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--leaves", type=int, default=32768)
ap.add_argument("--games", type=int, default=32768)
ap.add_argument("--prefill", type=int, default=600)
ap.add_argument("--steps", type=int, default=600)
ap.add_argument("--net", default=None, help="a tools/train_prior.py checkpoint (state_dict) to measure too")
ap.add_argument("--arena", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

N, WARM, ITERS, RANDOM_MOVES = 2, 20, 200, 30
GENBU_ARGS = dict(numMCTSSims=100, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5,
                  forced_playouts=False, dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
MODES = list(PRECISIONS)                                   # "f32" first: the others compare with it
dev = torch.device("cuda", 0)
eng = SplendorEngine(N, device=dev)
rb = RolloutBatch(eng, a.leaves, seed=7)
rb.run(RANDOM_MOVES)
state = eng.canonical(rb.state, rb.player)
mask = eng.valid_moves(state)

nets = {"random_init": random_net(N, seed=0, device=dev)}
if a.net and os.path.exists(a.net):
    net = random_net(N, seed=0, device=dev)
    data = torch.load(a.net, map_location=dev, weights_only=True)
    net.load_state_dict(data["state_dict"] if "state_dict" in data else data)
    nets["trained_prior"] = net.eval()

out = {"players": N, "leaves": a.leaves, "device": torch.cuda.get_device_name(dev),
       "timing": {"warmup_launches": WARM, "timed_launches": ITERS, "clock": "HIP events"},
       "full_batch_us": {}, "error_vs_float64": {}, "selfplay": {}}

# ---- full-batch time, all modes in this process, interleaved twice (the second pass is kept:
# clocks and caches settled for every mode alike)
evs = {m: LeafEvaluator(eng, nets["random_init"], a.leaves, use_graph=False, precision=m) for m in MODES}
for rep in range(2):
    for m in MODES:
        for _ in range(WARM):
            evs[m](state, mask)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(ITERS):
            evs[m](state, mask)
        e1.record()
        torch.cuda.synchronize(dev)
        out["full_batch_us"][m] = round(e0.elapsed_time(e1) / ITERS * 1e3, 2)
out["full_batch_speedup_vs_f32"] = {m: round(out["full_batch_us"]["f32"] / out["full_batch_us"][m], 3) for m in MODES}
print(json.dumps({"full_batch_us": out["full_batch_us"]}), flush=True)

# ---- error against float64
for name, net in nets.items():
    ev = LeafEvaluator(eng, net, a.leaves, use_graph=False)
    ev._convert(state, mask)
    with torch.no_grad():
        pi64, v64 = FoldedNet(net).to(dev).double().eval()(ev.x.double(), ev.valid, transposed=True)
    out["error_vs_float64"][name] = {}
    for m in MODES:
        pi, v = LeafEvaluator(eng, net, a.leaves, use_graph=False, precision=m)(state, mask)
        out["error_vs_float64"][name][m] = {"max_abs_pi": float((pi.double() - pi64).abs().max()),
                                            "mean_abs_pi": float((pi.double() - pi64).abs().mean()),
                                            "max_abs_v": float((v.double() - v64).abs().max()),
                                            "mean_abs_v": float((v.double() - v64).abs().mean())}
    del ev
print(json.dumps({"error_vs_float64": out["error_vs_float64"]}), flush=True)
del evs
torch.cuda.empty_cache()

# ---- self-play window per mode
from splendor.selfplay import SelfPlay  # noqa: E402
out["selfplay"] = {"games": a.games, "simulations": GENBU_ARGS["numMCTSSims"], "prefill_iterations": a.prefill,
                   "timed_iterations": a.steps, "network": "random_init", "modes": {}}
for m in MODES:
    ev = LeafEvaluator(eng, nets["random_init"], a.games, use_graph=False, precision=m)
    sp = SelfPlay(eng, a.games, GENBU_ARGS, evaluator=ev, dirichlet_noise=True, seed=0x5EED)
    sp.reset()
    sp.run(a.prefill, use_graph=True)
    sp.drain()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    sp.run(a.steps, use_graph=True)
    e1.record()
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    st = sp.stats()
    out["selfplay"]["modes"][m] = {"iter_ms_events": round(e0.elapsed_time(e1) / a.steps, 4),
                                   "sims_per_s": round(a.games * a.steps / wall),
                                   "overflow": st["overflow"], "prunes": st["prunes"], "resets": st["resets"],
                                   "unexpanded": st["unexpanded"], "moves": st["moves"]}
    print(json.dumps({"selfplay": {m: out["selfplay"]["modes"][m]}}), flush=True)
    del sp, ev
    torch.cuda.empty_cache()

# ---- arena record: one network, "bf16" against "f32"
if a.arena:
    from splendor.arena import BatchedArena  # noqa: E402
    from splendor.NNet import NNetWrapper  # noqa: E402
    from splendor.SplendorGame import SplendorGame  # noqa: E402
    game = SplendorGame(N)
    nn = NNetWrapper(game)
    which = "trained_prior" if "trained_prior" in nets else "random_init"
    nn.nnet.load_state_dict(nets[which].state_dict())
    nn.nnet.eval()
    args = dict(GENBU_ARGS, arenaCompare=256, nn_precision=("bf16", "f32"))
    t0 = time.perf_counter()
    one, two, draws = BatchedArena(game, nn, nn, args, batch=256).playGames(256)
    out["arena_bf16_vs_f32"] = {"network": which, "games": 256, "simulations": 100, "bf16_won": one, "f32_won": two,
                                "draws": draws, "seconds": round(time.perf_counter() - t0, 1)}

print(json.dumps(out), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
