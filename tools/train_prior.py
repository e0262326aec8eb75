#!/usr/bin/env python3
"""A trained 2-player prior for the benchmark's trained-prior regime: Coach.learn
(Coach.py:102-164, splendor/coach.py) on device self-play at genbu.pt's search arguments, from a
seeded random-init SplendorNNet, for a few iterations: numEps games per iteration on as many
concurrent trees, training on the example history (GenericNNetWrapper.train's losses and
schedule, larger batches), the BatchedArena gate against the previous weights. Writes the
accepted weights as a plain state_dict checkpoint ({"state_dict": ...}, weights-only loadable)
and one JSON line per iteration (losses, arena result, self-play figures) to stdout:
    python3 tools/train_prior.py OUT.pt [iterations] [games] [no-reserve] [bootstrap=K[:P]] [mix=L1,L2,..[:P]]
bench.py --net OUT.pt then runs the headline on these weights. A fourth argument `no-reserve`
plays the self-play games without the reserve moves 12..26 (args.selfplay_reserve = False,
the reference's training recipe); the arena gate still plays the full game. `bootstrap=K[:P]`
(anywhere after OUT.pt) plays the self-play of the first K iterations with the network-free
rollout search, P buy-first playouts per leaf (default 4; Coach.use_rollout_selfplay), on the
same trees and search arguments. `mix=L1,L2,...[:P]` plays iteration i (after the bootstrap) with
the mixed evaluator when Li is not 0: the network's priors, leaf values (1 - Li) v_network + Li
v_playout from P buy-first playouts (default 4; Coach.use_mixed_selfplay); iterations past the
list play on the network. Every iteration's line names the evaluator that played it."""
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))

from splendor.NNet import NNetWrapper  # noqa: E402
from splendor.SplendorGame import SplendorGame  # noqa: E402
from splendor.coach import Coach  # noqa: E402

bootstrap_iters, bootstrap_playouts = 0, 4
for arg in [x for x in sys.argv[1:] if x.startswith("bootstrap=")]:
    m = re.fullmatch(r"bootstrap=(\d+)(?::(\d+))?", arg)
    if not m:
        raise SystemExit(f"{arg}: expected bootstrap=ITERATIONS[:PLAYOUTS]")
    bootstrap_iters, bootstrap_playouts = int(m.group(1)), int(m.group(2) or 4)
    sys.argv.remove(arg)
mix, mix_playouts = [], 4
for arg in [x for x in sys.argv[1:] if x.startswith("mix=")]:
    m = re.fullmatch(r"mix=([0-9.,]+)(?::(\d+))?", arg)
    if not m:
        raise SystemExit(f"{arg}: expected mix=LAMBDA,LAMBDA,...[:PLAYOUTS]")
    mix, mix_playouts = [float(x) for x in m.group(1).split(",")], int(m.group(2) or 4)
    sys.argv.remove(arg)
out = sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/trained_2p.pt"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 4
games = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
if len(sys.argv) > 4 and sys.argv[4] != "no-reserve":
    raise SystemExit(f"{sys.argv[4]}: the fourth argument can only be no-reserve")
selfplay_reserve = len(sys.argv) <= 4
# (Coach.learn's checkpoints and example history stay out of gpurun_out: only OUT is kept)
folder = os.path.join(os.environ.get("TMPDIR", "/tmp"), "train_prior_ckpt")
g = SplendorGame(2)
torch.manual_seed(0)
nn = NNetWrapper(g, dict(epochs=2, batch_size=512, learn_rate=1e-3, dropout=0.3), seed=0)
args = dict(numMCTSSims=100, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5, forced_playouts=False,
            dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10, numIters=1, numEps=games,
            numItersHistory=3, arenaCompare=256, updateThreshold=0.55, checkpoint=folder,
            selfplay_reserve=selfplay_reserve)
coach = Coach(g, nn, args, batch=games, seed=0x7A11)
last = {}
orig_train = nn.train


def train(examples, **kw):
    r = orig_train(examples, **kw)
    last["losses"] = r
    last["examples"] = len(examples)
    return r


nn.train = train
pnet = NNetWrapper(g, dict(nn.args), device=nn.device)
accepted = 0
for i in range(1, iters + 1):
    t0 = time.perf_counter()
    played = "network"
    if i <= bootstrap_iters:                                # (learn() puts the network back afterwards)
        ev = coach.use_rollout_selfplay(playouts=bootstrap_playouts)
        played = f"rollout:{ev.policy}:{ev.playouts}"
    elif i <= len(mix) and mix[i - 1] != 0:
        ev = coach.use_mixed_selfplay(mix[i - 1], playouts=mix_playouts)
        played = f"mixed:{ev.lam}:{ev.policy}:{ev.playouts}"
    (nw, pw, dr, ok), = coach.learn(pnet=pnet)
    accepted += bool(ok)
    st = coach.sp.stats()
    print(json.dumps({"iteration": i, "seconds": time.perf_counter() - t0, "examples": last.get("examples"),
                      "losses": {k: float(v) for k, v in (last.get("losses") or {}).items()},
                      "arena_new_prev_draws": [nw, pw, dr], "accepted": bool(ok), "selfplay_evaluator": played,
                      "selfplay_leaf_depth_now": st["leaf_depth_now"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
torch.save({"state_dict": nn.nnet.state_dict(), "iterations": iters, "accepted": accepted}, out)
print(json.dumps({"saved": out, "iterations": iters, "accepted": accepted, "bootstrap_iters": bootstrap_iters,
                  "bootstrap_playouts": bootstrap_playouts, "mix": mix, "mix_playouts": mix_playouts}), flush=True)
