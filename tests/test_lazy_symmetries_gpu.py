"""Lazy symmetry expansion on the device: spl_symmetry_counts and the batch-assembly kernel
spl_gather_examples against the reference-executed fixtures (tests/golden/sym_*p.npz, the
reference's own get_symmetries output, independent of k_symmetries), against
materialize() + index_select, the index guard, training on a lazy set, and the Coach path."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_lazy_symmetries import base_set, fixture  # noqa: E402

pytestmark = pytest.mark.gpu

COLS = ("board", "pi", "winner", "scdiff", "valids", "surprise")


@functools.lru_cache(maxsize=None)
def setup(n):
    """(fixture arrays, engine, lazy set on the device, its materialised form): built once
    per player count and never modified."""
    from splendor.env import SplendorEngine
    from splendor.examples import LazySymmetryExamples
    d = fixture(n)
    e = SplendorEngine(n)
    lz = LazySymmetryExamples(base_set(d, n).to(e.device), e)
    return d, e, lz, lz.materialize()


def reference_rows(mat, ids):
    """What train's materialised path feeds the network for rows `ids`."""
    from splendor.env import unpack_mask
    return (mat.board.index_select(0, ids).float(), mat.pi.index_select(0, ids), mat.winner.index_select(0, ids),
            mat.scdiff.index_select(0, ids), unpack_mask(mat.valids.index_select(0, ids)))


def assert_same(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert torch.equal(g, w), k


@pytest.mark.parametrize("n", (2, 3, 4))
def test_counts_match_reference(n):
    d, e, lz, _ = setup(n)
    counts = e.symmetry_counts(torch.from_numpy(d["src"]).to(e.device))
    assert counts.dtype == torch.uint8
    np.testing.assert_array_equal(counts.cpu().numpy(), np.diff(d["off"]))
    assert torch.equal(lz.counts, counts) and len(lz) == len(d["state"])
    assert e.symmetry_counts(torch.empty((0, e.rows, 7), dtype=torch.int8, device=e.device)).shape == (0,)


@pytest.mark.parametrize("n", (2, 3, 4))
def test_every_row_in_order_matches_reference(n):
    d, e, lz, _ = setup(n)
    total = len(d["state"])
    x, pi, winner, scdiff, valids = lz.batch(torch.arange(total, device=e.device))
    lz.check_errors()
    assert x.dtype == torch.float32 and x.shape == (total, e.rows, 7)
    assert valids.dtype == torch.bool and valids.shape == (total, 409)
    assert torch.equal(x.cpu(), torch.from_numpy(d["state"]).float())
    assert torch.equal(pi.cpu(), torch.from_numpy(d["pi"]))
    assert torch.equal(valids.cpu(), torch.from_numpy(d["valids"]).bool())
    owner = torch.from_numpy(np.repeat(np.arange(40), np.diff(d["off"]))).to(e.device)
    assert torch.equal(winner, lz.base.winner[owner]) and winner.dtype == torch.float32
    assert torch.equal(scdiff, lz.base.scdiff[owner]) and scdiff.dtype == torch.int32


@pytest.mark.parametrize("n", (2, 3, 4))
@pytest.mark.parametrize("M", (1, 5, 67))
def test_odd_batches_match_materialized(n, M):
    """Sizes that are no multiple of the 4 waves per block, rows shuffled with repeats."""
    d, e, lz, mat = setup(n)
    assert len(mat) == len(lz)
    g = torch.Generator().manual_seed(1000 * n + M)
    ids = torch.randint(0, len(lz), (M,), generator=g)
    if M > 2:
        ids[M // 2] = ids[0]                      # a repeated row
    ids = ids.to(e.device)
    assert_same(lz.batch(ids), reference_rows(mat, ids))
    lz.check_errors()


def test_index_guard():
    """One row names example E, one the variant just past its position's last: both come
    back as zeros, the error bit is set, every other row is right. The source columns hold
    a spare row beyond E, so the out-of-range example is allocated memory either way; no
    negative or large index is used."""
    from splendor import _lib
    d, e, lz, mat = setup(2)
    E, b = lz.n_base, lz.base
    cols = [torch.cat([getattr(b, k), getattr(b, k)[:1]]).contiguous()
            for k in ("board", "pi", "valids", "winner", "scdiff")]
    assert all(c.shape[0] == E + 1 for c in cols)
    counts = lz.counts.cpu().numpy()
    short = int(np.flatnonzero(counts < 10 + 2 * 2)[0])           # a position with fewer than K variants
    example = torch.tensor([3, 7, E, 11, short, short, E - 1], dtype=torch.int64, device=e.device)
    ordinal = torch.tensor([0, 13, 0, 5, int(counts[short]), int(counts[short]) - 1, int(counts[E - 1]) - 1],
                           dtype=torch.int32, device=e.device)
    bad = [2, 4]
    err = torch.zeros(1, dtype=torch.int32, device=e.device)
    x, pi, valid, winner, scdiff = e.gather_examples(*cols, example, ordinal, err=err, rows=E)
    assert int(err.item()) == _lib.ERR_BAD_INDEX
    for t in (x, pi, valid, winner, scdiff):
        assert not bool(t[bad].any())
    good = [i for i in range(len(example)) if i not in bad]
    rows = (lz.offsets[example[good]] + ordinal[good]).to(torch.int64)
    want = reference_rows(mat, rows)
    assert_same((x[good], pi[good], winner[good], scdiff[good], valid[good]), want)
    # the lazy set reports the same condition once, at check_errors()
    lz.batch(torch.tensor([len(lz)], device=e.device))
    with pytest.raises(IndexError):
        lz.check_errors()
    lz.check_errors()                                              # cleared


def _train(examples, sample_ids, nn_args, **kw):
    """One train call on a fresh, identically seeded network; returns the tensors every
    step handed to NNetWrapper.losses and the per-step losses."""
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame
    w = NNetWrapper(SplendorGame(2), nn_args, seed=0)
    w._loss_log = []
    seen, inner = [], w.losses

    def spy(*a):
        seen.append([t.detach().clone() for t in a])
        return inner(*a)
    w.losses = spy
    torch.manual_seed(1)
    w.train(examples, sample_ids=sample_ids, **kw)
    return seen, np.array(w._loss_log)


def test_training_sees_the_same_tensors():
    """symmetry_sampling='all' (default): with the same injected sample_ids the lazy set
    hands NNetWrapper.losses bit-identical tensors at every step, and the per-step losses
    agree within the run-to-run difference of the materialised path on the same inputs
    (measured here; 0 when the training step is deterministic)."""
    d, e, lz, mat = setup(2)
    nn_args = dict(epochs=1, batch_size=32, dropout=0.0)
    steps = len(lz) // 32
    assert steps == 539 // 32 == 16
    rng = np.random.default_rng(11)
    ids = [rng.choice(len(lz), 32, replace=False) for _ in range(steps)]
    seen_a, loss_a = _train(mat, ids, nn_args)
    seen_b, loss_b = _train(mat, ids, nn_args)
    seen_l, loss_l = _train(lz, ids, nn_args)
    assert len(seen_a) == len(seen_l) == steps and loss_l.shape == loss_a.shape == (steps, 4)
    for sa, sl in zip(seen_a, seen_l):
        assert_same(sl, sa)
    tol = float(np.abs(loss_a - loss_b).max())
    diff = float(np.abs(loss_l - loss_a).max())
    print(f"materialised run-to-run max |dloss| = {tol:g}, lazy vs materialised = {diff:g}")
    assert diff <= tol


def test_symmetry_sampling_one(monkeypatch):
    """Opt-in sampling over stored positions: n_base // batch_size steps per epoch, each
    position at most once per batch, ordinals below the position's count, reproducible
    from the generator seed, and injected ordinals honoured."""
    from splendor.examples import LazySymmetryExamples
    d, e, lz, mat = setup(2)
    calls, inner = [], LazySymmetryExamples.batch_pairs

    def spy(self, example, ordinal):
        calls.append((example.cpu().clone(), ordinal.cpu().clone()))
        return inner(self, example, ordinal)
    monkeypatch.setattr(LazySymmetryExamples, "batch_pairs", spy)
    monkeypatch.setattr(LazySymmetryExamples, "batch", lambda self, rows: pytest.fail("row-space batch in 'one' mode"))
    nn_args = dict(epochs=2, batch_size=8, dropout=0.0, symmetry_sampling="one")
    steps = lz.n_base // 8
    counts = lz.counts.cpu()

    def run(seed):
        calls.clear()
        gen = torch.Generator(device=e.device)
        gen.manual_seed(seed)
        seen, losses = _train(lz, None, nn_args, generator=gen)
        assert len(seen) == len(calls) == len(losses) == 2 * steps == 10
        return list(calls)
    first = run(5)
    for ex, od in first:
        assert ex.shape == od.shape == (8,)
        assert bool((ex >= 0).all()) and bool((ex < lz.n_base).all())
        assert len(set(ex.tolist())) == 8                                   # a batch: without replacement
        assert bool((od >= 0).all()) and bool((od < counts[ex]).all())
    assert any(bool((od > 0).any()) for _, od in first)
    again = run(5)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again))
    other = run(6)
    assert any(not torch.equal(a[0], b[0]) or not torch.equal(a[1], b[1]) for a, b in zip(first, other))
    # injected rows and ordinals
    rng = np.random.default_rng(3)
    ids = [rng.choice(lz.n_base, 8, replace=False) for _ in range(2 * steps)]
    ords = [(rng.integers(0, 1 << 16, 8) % counts.numpy()[i]).astype(np.int32) for i in ids]
    calls.clear()
    seen, _ = _train(lz, ids, nn_args, sample_variants=ords)
    assert len(calls) == 2 * steps
    for (ex, od), i, o in zip(calls, ids, ords):
        np.testing.assert_array_equal(ex.numpy(), i)
        np.testing.assert_array_equal(od.numpy(), o)
    rows = torch.from_numpy(np.concatenate(ids)).to(e.device)
    rows = lz.offsets[rows] + torch.from_numpy(np.concatenate(ords)).to(e.device)
    want = reference_rows(mat, rows)
    got = [torch.cat([s[k] for s in seen]) for k in range(5)]
    assert_same(got, want)
    with pytest.raises(ValueError):
        _train(lz, ids, dict(nn_args, symmetry_sampling="all"), sample_variants=ords)


def test_coach_lazy_iteration(tmp_path):
    """Coach with lazy_symmetries: the same self-play as the default coach, stored
    unexpanded (materialize() gives the expanded set bit for bit; the device queue order is
    not fixed, so both sides are ordered by content), then learn() end to end on the lazy
    path and a history file that holds the stored positions only."""
    from splendor.NNet import NNetWrapper
    from splendor.SplendorGame import SplendorGame
    from splendor.coach import Coach
    from splendor.examples import ExampleSet, LazySymmetryExamples
    from splendor.mcts import HashEvaluator
    args = dict(numMCTSSims=8, cpuct=1.5, fpu=0.1, prob_fullMCTS=1.0, ratio_fullMCTS=4,
                forced_playouts=False, dirichletAlpha=0.0, temperature=[1.25, 0.8], tempThreshold=10,
                numItersHistory=2, numIters=1, numEps=2, arenaCompare=2, updateThreshold=0.55,
                checkpoint=str(tmp_path))

    def coach(**kw):
        g = SplendorGame(2)
        c = Coach(g, None, dict(args, **kw), batch=16, seed=5, mem_budget=1 << 30)
        c.sp.evaluator = HashEvaluator(g.engine)
        return c

    lazy = coach(lazy_symmetries=True).executeIteration(2)
    full = coach().executeIteration(2)
    assert isinstance(lazy, LazySymmetryExamples) and type(full) is ExampleSet
    assert len(lazy) == len(full) > lazy.n_base > 0
    assert 10 * lazy.n_base <= len(lazy) <= 14 * lazy.n_base
    key = lambda t: (t[0].tobytes(), t[1].tobytes())
    got, want = sorted(lazy.materialize().to_tuples(), key=key), sorted(full.to_tuples(), key=key)
    for x, y in zip(got, want):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)

    g = SplendorGame(2)
    nn = NNetWrapper(g, dict(epochs=1, batch_size=32))
    c = Coach(g, nn, dict(args, lazy_symmetries=True), batch=16, seed=4, mem_budget=1 << 30)
    hist = c.learn()
    assert len(hist) == 1 and sum(hist[0][:3]) == 2
    h = c.trainExamplesHistory
    assert h.is_lazy() and len(h.iters) == 1 and len(h) >= 32
    n_base = h.merged().n_base
    with np.load(os.path.join(str(tmp_path), "checkpoint.examples.npz"), allow_pickle=False) as z:
        assert int(z["format"]) == 2 and str(z["symmetries"]) == "lazy"
        assert z["board"].shape[0] == z["pi"].shape[0] == n_base == int(z["sizes"].sum())
    c.loadTrainExamples(str(tmp_path))
    back = c.trainExamplesHistory.merged()
    assert isinstance(back, LazySymmetryExamples) and back.device.type == "cuda"
    assert back.n_base == n_base and len(back) == len(h)
    for k in COLS:
        assert torch.equal(getattr(back.base, k), getattr(h.merged().base, k)), k
