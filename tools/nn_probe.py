#!/usr/bin/env python3
"""k_nn_forward per-layer cycle probes over a full batch (diagnostic): the
library named by SPLENDOR_AMD_LIB built with -DNN_PROBE=1 (wave 0 of every workgroup stamps
each layer boundary), B = 32,768 leaves of mid-game positions, a seeded random-init network;
prints the average cycles per workgroup of each stage.
  SPLENDOR_AMD_LIB=$PWD/ablib/libnnprobe.so python3 tools/nn_probe.py [B] [players] [full|indexed|staged]
full: rows 0 .. B (no list); indexed / staged: every row listed, through spl_nn_forward_indexed
or through the staged leaf buffer (filled once by spl_nn_stage_leaves) — the two input paths
of the search, on the same leaves and tiles."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))

from splendor import _lib  # noqa: E402
from splendor.env import RolloutBatch, SplendorEngine  # noqa: E402
from splendor.nnet import LeafEvaluator, random_net  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2
MODE = sys.argv[3] if len(sys.argv) > 3 else "full"
assert MODE in ("full", "indexed", "staged"), MODE
dev = torch.device("cuda", 0)
eng = SplendorEngine(N, device=dev)
rb = RolloutBatch(eng, B, seed=7)
rb.run(30)
state = eng.canonical(rb.state, rb.player)
mask = eng.valid_moves(state)
ev = LeafEvaluator(eng, random_net(N, seed=0, device=dev), B, use_graph=False)
L = _lib.lib()
L.spl_diag_nn_probe.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
out = (ctypes.c_ulonglong * 16)()
how = {}
if MODE == "indexed":
    how = dict(index=torch.arange(B, dtype=torch.int32, device=dev),
               count=torch.full(((B + 63) // 64,), 64, dtype=torch.int32, device=dev))
    how["count"][-1] = B - 64 * ((B - 1) // 64)
elif MODE == "staged":
    from splendor.env import _ptr  # noqa: E402
    from splendor.nnet import new_stage  # noqa: E402
    how = dict(stage=new_stage(N, B, dev))
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    _lib.check(L.spl_nn_stage_leaves(eng.ctx, B, _ptr(state), _ptr(ones), _ptr(torch.zeros_like(mask)),
                                     _ptr(how["stage"]), eng._s()), "spl_nn_stage_leaves")
for _ in range(5):
    ev(state, mask, **how)
torch.cuda.synchronize(dev)
L.spl_diag_nn_probe(out, 1)
for _ in range(20):
    ev(state, mask, **how)
torch.cuda.synchronize(dev)
L.spl_diag_nn_probe(out, 0)
wg = max(int(out[15]), 1)
names = ("input", "dense2d_1", "dense2d_1[3]", "partialgpool_1", "dense2d_3+flatten", "dense1d_4", "pgp4..pgp5",
         "heads_PI0_V0", "PI1_V1", "softmax")
per = {n: out[k] / wg for k, n in enumerate(names)}
print(json.dumps({"B": B, "players": N, "mode": MODE, "workgroups": wg, "cycles_per_workgroup": per,
                  "total": sum(per.values())}, indent=1))
