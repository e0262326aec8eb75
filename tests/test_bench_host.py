"""Host logic of bench.py (no GPU): the phase-stagger schedule and the algorithmic byte and
FLOP figures its roofline blocks are built on."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("cfg,stagger", [("config3", 4800), ("config5", 32000), ("config4", 40000)])
def test_stagger_marks_stay_on_the_search_grid(bench, cfg, stagger):
    n, B, sims = bench.CONFIGS[cfg]
    ratio = bench.GENBU_ARGS["ratio_fullMCTS"]
    marks = bench.stagger_marks(stagger, 16, sims, ratio)
    its = [i for i, _ in marks]
    assert [j for _, j in marks] == list(range(1, 16))
    assert all(i % (sims // ratio) == 0 for i in its)        # restarts on search boundaries
    assert its == sorted(set(its)) and 0 < its[0] and its[-1] < stagger
    assert its[-1] + its[0] >= stagger - 16 * (sims // ratio)   # spread over ~the whole span


def test_stagger_marks_empty_when_too_short(bench):
    assert bench.stagger_marks(100, 16, 100, 5) == []
    assert bench.stagger_marks(0, 16, 100, 5) == []


def test_algorithmic_figures(bench):
    assert bench.bytes_per_board_step(2) == 846                  # SURVEY §8(d), 2 players
    assert round(bench.bytes_per_rollout(2, 4.8)) == 3698        # ~3.7 KB per simulation
    assert bench.nn_flops_per_eval(2) == 2 * 595328              # 1.19 MFLOP per leaf


def _run_bench(argv, env_extra=None, timeout=240):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_gpus_flag_launches_that_many_ranks():
    """`bench.py --gpus 2` without torch.distributed.run starts 2 ranks itself (gloo dry run:
    barrier, max over ranks) and rank 0 prints ONE JSON line with n_gpus 2."""
    import json
    r = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_reporting"] == 2 and out["steps"] == 3 and out["dry_run"]


def test_gpus_flag_must_match_world_size():
    r = _run_bench(["--gpus", "2", "--dry-run"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE 1" in r.stderr


@pytest.mark.parametrize("workload", ["config4", "all"])
def test_config4_multi_rank_dry_run(workload):
    """BASELINE config 4 at N = 2: the run measures config 4's per-GPU shard
    on every rank (65,536 games in all) with its own prefill / stagger / window, and its
    window's example all-gather runs over the ranks (gloo here, RCCL on the GPUs)."""
    import json
    argv = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", workload, "--dry-run"]
    if workload == "all":
        plain = _run_bench(argv)                        # the secondary objects are behind --full
        assert plain.returncode == 0, plain.stderr[-2000:]
        assert "config4_shard" not in json.loads([ln for ln in plain.stdout.splitlines() if ln.startswith("{")][-1])
        argv.append("--full")
    r = _run_bench(argv)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    c4 = out["selfplay"] if workload == "config4" else out["config4_shard"]
    assert out["n_gpus"] == 2 and c4["n_gpus"] == 2 and c4["global_games"] == 65536
    assert c4["window"]["examples_gathered"] == 3 + 4          # rank 0: 3 examples, rank 1: 4
    assert (c4["window"]["prefill"], c4["window"]["stagger"], c4["window"]["window"]) == (84000, 80000, 4000)
    if workload == "all":
        assert out["selfplay"]["global_games"] == 65536 and out["selfplay"]["numMCTSSims"] == 100


def test_phase_defaults_per_workload(bench):
    assert bench.PHASES["config3"] == dict(prefill=6000, stagger=4800, window=10000)
    assert bench.PHASES["config4"]["prefill"] == 84000 and bench.PHASES["config5"]["prefill"] == 40000


def test_dump_outputs_ignores_queue_order(bench, tmp_path):
    """--dump-outputs (host part, stub engine on the CPU): the arrays are float32 / float64
    .npy files, and the example sample does not depend on the order in which the finished
    examples stand in the queue (games that end in one iteration take their slots in any
    order): two queue orders give the same files."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    from splendor.mcts import HDR_DTYPE
    B, n, R, E = 96, 2, 56, 5000
    g = torch.Generator().manual_seed(1)
    hdr = np.zeros(B, HDR_DTYPE)
    for f in bench.DUMP_HEADER_FIELDS:
        hdr[f] = np.arange(B) * 3 + len(f)
    sp = SimpleNamespace(B=B, e=SimpleNamespace(device=torch.device("cpu")), headers=lambda: hdr,
                         root_stats=lambda: (torch.arange(B * 409).reshape(B, 409),
                                             torch.rand((B, 409), generator=g, dtype=torch.float64),
                                             torch.rand((B, 409), generator=g, dtype=torch.float64),
                                             torch.rand((B, n), generator=g, dtype=torch.float64)),
                         leaf_state=torch.randint(0, 9, (B, R, 7), generator=g).to(torch.int8))
    ev = SimpleNamespace(pi_buf=torch.rand((B, 409), generator=g), v_buf=torch.rand((B, n), generator=g))
    meta = torch.stack([torch.arange(E) // 50, torch.arange(E) % 50 // 10, torch.arange(E) % 10,
                        torch.arange(E) % n], 1).to(torch.int32)
    ex = {"meta": meta, "board": torch.randint(0, 9, (E, R, 7), generator=g).to(torch.int8),
          "pi": torch.rand((E, 409), generator=g), "valids": torch.randint(-2**62, 2**62, (E, 7), generator=g),
          "winner": torch.rand((E, n), generator=g), "scdiff": torch.randint(-9, 9, (E, n), generator=g).to(torch.int32),
          "surprise": torch.rand((E, n), generator=g)}
    perm = torch.randperm(E, generator=g)
    for d, e in (("a", ex), ("b", {k: v[perm] for k, v in ex.items()})):
        g.manual_seed(2)                                   # (the stub's root_stats draw from g)
        bench.dump_selfplay_outputs(sp, ev, e, str(tmp_path / d), 0x5EED)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "example_pi.npy" in names and "root_counts.npy" in names
    total = 0
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), nm
        total += a.nbytes
    assert total <= 64 << 20
    m = np.load(tmp_path / "a" / "example_meta.npy")
    assert m.shape == (bench.DUMP_EXAMPLES, 4)
    keys = m[:, 0] * 1e6 + m[:, 1] * 1e3 + m[:, 2]
    assert (np.diff(keys) > 0).all()                       # sorted by (board id, game, move), no repeats
    v = np.load(tmp_path / "a" / "example_valids.npy")
    row = int(np.flatnonzero((meta[:, :3].numpy() == m[0, :3]).all(1))[0])
    word, bit = divmod(70, 64)
    assert v.shape == (bench.DUMP_EXAMPLES, 409) and v[0, 70] == (int(ex["valids"][row, word]) >> bit) & 1
    assert np.load(tmp_path / "a" / "tree_headers.npy").shape == (B, len(bench.DUMP_HEADER_FIELDS))


def test_window_counters_are_wrap_safe():
    """the per-tree 32-bit header counters (depth_sum wraps after ~40 M simulations
    of a long-lived tree) are differenced per tree modulo 2^32 before summing."""
    import numpy as np
    from splendor.selfplay import SelfPlay
    before = {"depth_sum": np.array([2**32 - 10, 5, 2**31 - 1], np.uint32)}
    after = {"depth_sum": np.array([20, 9, 2**31 + 99], np.uint32)}
    assert SelfPlay.counter_delta(before, after) == {"depth_sum": 30 + 4 + 100}
