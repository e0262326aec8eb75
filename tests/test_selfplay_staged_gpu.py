"""Self-play through the staged leaf buffer (spl_mcts_select_staged + spl_nn_forward_staged,
the default) plays exactly the games of the indexed path (SPLENDOR_NN_STAGED=0:
spl_mcts_select_compact + spl_nn_forward_indexed): same seed, same network, each run in a fresh
child process (the switch is read when splendor.mcts is imported); tree headers, root statistics
and the drained examples sorted by (board, game, move) bit-identical, no capacity events."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SIMS, ITERS = 192, 16, 448
HDR = ("player", "episode_step", "move_no", "game_no", "games_done", "moves", "sims_done", "depth", "full",
       "budget", "depth_sum", "sims_backed")


def _child(n, out):
    sys.path[:0] = [os.path.join(ROOT, "alphazero-general-ori_amd")]
    import torch
    from splendor.env import SplendorEngine
    from splendor.nnet import LeafEvaluator, random_net
    from splendor.selfplay import SelfPlay
    args = dict(numMCTSSims=SIMS, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=8, forced_playouts=False,
                dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
    e = SplendorEngine(n, device="cuda:0")
    ev = LeafEvaluator(e, random_net(n, seed=3, device="cuda:0"), B, use_graph=False)
    sp = SelfPlay(e, B, args, evaluator=ev, seed=0x5EED, mem_budget=1 << 30)
    sp.reset()
    sp.run(ITERS, use_graph=True)
    torch.cuda.synchronize()
    h = sp.headers()
    counts, qsa, probs, q = sp.root_stats()
    ex = sp.drain()
    order = np.lexsort(ex["meta"].cpu().numpy()[:, :3].T[::-1])       # by (board, game, move)
    arrays = {f"hdr_{k}": h[k] for k in HDR}
    arrays.update(counts=counts.cpu().numpy(), qsa=qsa.cpu().numpy(), probs=probs.cpu().numpy(), q=q.cpu().numpy())
    arrays.update({f"ex_{k}": v.cpu().numpy()[order] for k, v in ex.items()})
    arrays["staged"] = np.array([sp.stage is not None])
    arrays["events"] = np.array([sum(sp.capacity_events().values()), sp.dropped_examples()])
    np.savez(out, **arrays)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (2, 4))
def test_staged_selfplay_equals_indexed(n, tmp_path):
    runs = []
    for staged in ("1", "0"):
        out = str(tmp_path / f"run{staged}.npz")
        env = dict(os.environ, SPLENDOR_NN_STAGED=staged)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), out], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(out) as z:
            runs.append({k: z[k] for k in z.files})
    a, b = runs
    assert bool(a["staged"][0]) and not bool(b["staged"][0])           # the two paths did run
    assert a["events"].tolist() == [0, 0] and b["events"].tolist() == [0, 0]
    assert int(a["hdr_moves"].sum()) > B                               # (searches finished, moves played)
    print(f"{n} players: {int(a['hdr_moves'].sum())} moves, {len(a['ex_meta'])} examples drained")
    assert sorted(a) == sorted(b)
    for k in a:
        if k != "staged":
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
