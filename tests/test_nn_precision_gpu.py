"""Reduced-precision modes of the fused network kernel on the GPU (spl_nn_forward_mode):
the kernel against the host definition (splendor.nnet.reduced_forward) on the conditioned
fixture, mode 0 against the existing entry points bit for bit, tiles / segmented lists in the
reduced modes bit for bit against themselves (random-init networks: bit-equality needs no
conditioning, tolerances on them mean nothing), and a short self-play run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_nn_precision import fixture_forward
from test_nnet import _pack_mask, deterministic_weights

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REDUCED = ("bf16x2", "bf16")

# Kernel vs reduced_forward on the 12 fixture boards: tau(mode) = (pi, v). Each is 4 x the maximum
# measured on an MI355X over n = 2, 3, 4 (MEASURED, same layout), capped at a quarter of the
# mode's own fixture distance from "f32" (CAP: 8.3e-6 / 9.4e-4 for bf16, 3.2e-8 / 4.0e-6 for
# bf16x2), so a wrong mode, a dropped or added product or a truncation in the wrong place fails.
CAP = {"bf16": (2.0e-6, 2.3e-4), "bf16x2": (8e-9, 1.0e-6)}
MEASURED = {"bf16": (7.2e-10, 2.1e-8), "bf16x2": (2.7e-9, 1.22e-7)}
TAU = {m: tuple(min(c, 4 * x) for c, x in zip(CAP[m], MEASURED[m])) for m in CAP}


def fixture_net(n):
    from splendor.nnet import SplendorNNet
    with np.load(os.path.join(GOLD, f"nnet_{n}p.npz")) as z:
        g = {k: z[k] for k in z.files}
    net = SplendorNNet(n)
    net.load_state_dict(deterministic_weights(net.state_dict()))
    boards = torch.from_numpy(np.ascontiguousarray(g["boards"].astype(np.int8))).cuda()
    mask = torch.from_numpy(_pack_mask(g["valid"])).cuda()
    return net.cuda().eval(), boards, mask


def forward_mode(fused, boards, mask, mode, pi=None, v=None, index=None, count=None):
    """spl_nn_forward_mode itself (FusedNet's "f32" goes through the two older entry points)."""
    from splendor import _lib
    from splendor.env import ACTIONS, _ptr
    B = boards.shape[0]
    pi = pi if pi is not None else torch.empty((B, ACTIONS), dtype=torch.float32, device="cuda")
    v = v if v is not None else torch.empty((B, fused.n), dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().spl_nn_forward_mode(fused.n, B, _ptr(boards), _ptr(mask), _ptr(index), _ptr(count),
                                              _ptr(fused.w), _ptr(pi), _ptr(v), mode, s), "spl_nn_forward_mode")
    return pi, v


def env_batch(n, B, seed):
    """B real boards (golden env states, some perturbed) and masks, row 3 with no valid move."""
    with np.load(os.path.join(GOLD, f"env_{n}p.npz")) as z:
        st, mk = z["state"], z["mask_player"]
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(st), B)
    boards = st[idx].copy()
    boards[::7] = rng.integers(-20, 20, boards[::7].shape)
    valid = mk[idx].astype(bool)
    valid[3] = False
    return torch.from_numpy(boards).cuda(), torch.from_numpy(_pack_mask(valid)).cuda()


@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("n", (2, 3, 4))
def test_reduced_kernel_matches_definition(n, mode):
    """The kernel in a reduced mode on the 12 fixture boards (one partial tile; 3 players: a
    board size that is no multiple of 4 bytes) equals reduced_forward within TAU."""
    from splendor.nnet import FusedNet
    net, boards, mask = fixture_net(n)
    pi, v = FusedNet(net, n, "cuda", precision=mode)(boards, mask)
    rpi, rv = fixture_forward(n, mode)
    dpi = np.abs(pi.double().cpu().numpy() - rpi).max()
    dv = np.abs(v.double().cpu().numpy() - rv).max()
    print(f"n={n} {mode}: kernel vs definition max|dpi|={dpi:.3e} max|dv|={dv:.3e} (tau {TAU[mode]})")
    assert dpi <= TAU[mode][0]
    assert dv <= TAU[mode][1]


@pytest.mark.parametrize("n", (2, 3, 4))
def test_mode_f32_is_the_existing_kernel(n):
    """spl_nn_forward_mode(SPL_NN_F32) is bit-identical to spl_nn_forward and, with a list, to
    spl_nn_forward_indexed (listed rows written, the others untouched)."""
    from splendor.nnet import FusedNet, random_net
    B = 3 * 32 + 5
    boards, mask = env_batch(n, B, 30 + n)
    fused = FusedNet(random_net(n, seed=7), n, "cuda")
    pi0, v0 = fused(boards, mask)
    pi1, v1 = forward_mode(fused, boards, mask, 0)
    assert torch.equal(pi0, pi1) and torch.equal(v0, v1)
    index, count, rows = segmented_list(B, (17, 1), seed=n)
    out = []
    for call in (fused, lambda *a, **k: forward_mode(fused, *a[:2], 0, *a[2:], **k)):
        pi = torch.full((B, 409), -7.0, device="cuda")
        v = torch.full((B, n), -7.0, device="cuda")
        call(boards, mask, pi, v, index=index, count=count)
        out.append((pi, v))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[1][0][rows], pi0[rows]) and torch.equal(out[1][1][rows], v0[rows])


def segmented_list(B, counts, seed):
    """The search's NN-leaf list over ceil(B / 64) segments with the given counts: entries of a
    segment in reverse order, -1 behind them. Returns (index, count, listed rows) on the GPU."""
    rng = np.random.default_rng(seed)
    nseg = (B + 63) // 64
    assert len(counts) == nseg
    index_np = np.full(B, -1, dtype=np.int32)
    rows = []
    for j, c in enumerate(counts):
        size = min(64, B - 64 * j)
        r = np.sort(rng.choice(size, c, replace=False)).astype(np.int32)[::-1] + 64 * j
        index_np[64 * j:64 * j + c] = r
        rows.append(r)
    rows = np.concatenate(rows).astype(np.int64)
    return (torch.from_numpy(index_np).cuda(), torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda(),
            torch.from_numpy(rows).cuda())


@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("n", (2, 3))
def test_reduced_kernel_tiles_and_lists(n, mode):
    """A reduced mode over 3 tiles and a partial one (random-init network, real boards): every row
    is bit-identical to the same board in a single-tile launch, whatever its place in the tile;
    the segmented form (2 segments, one of count 1 or 0, entries reversed, sentinel-filled
    outputs) writes exactly the listed rows, bit-identical to the full batch; the row with no
    valid move is finite like the rest."""
    from splendor.nnet import FusedNet, random_net
    B = 3 * 32 + 5
    boards, mask = env_batch(n, B, 40 + n)
    fused = FusedNet(random_net(n, seed=8), n, "cuda", precision=mode)
    pi, v = fused(boards, mask)
    pi, v = pi.clone(), v.clone()
    assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all())
    np.testing.assert_allclose(pi.sum(1).cpu().numpy(), 1.0, atol=1e-5)
    assert bool((v.abs() <= 1).all())
    for s in (0, 32, 64, 96, 13, 69, 90):                  # single-tile launches (partial: 96, 90)
        k = min(32, B - s)
        p1, v1 = fused(boards[s:s + k].contiguous(), mask[s:s + k].contiguous())
        assert torch.equal(p1, pi[s:s + k]) and torch.equal(v1, v[s:s + k]), s
    # the mode is not the exact kernel under another name
    pe, _ = forward_mode(fused, boards, mask, 0)
    assert not torch.equal(pe, pi)
    for counts in ((1, 20), (40, 0)):
        index, count, rows = segmented_list(B, counts, seed=n)
        po = torch.full((B, 409), -7.0, device="cuda")
        vo = torch.full((B, n), -7.0, device="cuda")
        fused(boards, mask, po, vo, index=index, count=count)
        assert torch.equal(po[rows], pi[rows]) and torch.equal(vo[rows], v[rows]), counts
        other = torch.ones(B, dtype=torch.bool, device="cuda")
        other[rows] = False
        assert bool((po[other] == -7.0).all()) and bool((vo[other] == -7.0).all()), counts


SEARCH_ARGS = dict(numMCTSSims=25, cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5, forced_playouts=False,
                   dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)


def selfplay_run(make_evaluator):
    from splendor.env import SplendorEngine
    from splendor.selfplay import SelfPlay
    e = SplendorEngine(2)
    ev = make_evaluator(e)
    sp = SelfPlay(e, 64, SEARCH_ARGS, evaluator=ev, dirichlet_noise=True, seed=0x5EED, mem_budget=1 << 30)
    sp.reset()
    sp.run(40, use_graph=True)
    torch.cuda.synchronize()
    h = sp.headers().copy()
    counts = sp.root_stats()[0].cpu().numpy()
    ex = {k: t.cpu().numpy() for k, t in sp.drain().items()}
    priors = ev.pi_buf.cpu().numpy()         # (every row written: the first iteration expands all roots)
    return h, counts, ex, sp.capacity_events(h), priors


def assert_same_run(a, b):
    for k in ("player", "episode_step", "move_no", "game_no", "games_done", "moves", "sims_done", "depth",
              "overflow", "n_examples"):
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=k)


def test_selfplay_precision_argument():
    """SelfPlay, 2 players, 64 games, 25 simulations, 40 iterations. precision="f32" through the
    new argument plays the default construction's run (headers, root visit counts, drained
    examples). With "bf16": two runs from one seed are identical, no tree's error word
    (header `overflow`) is set, there are no capacity events, and every policy row — the drained
    examples' and the priors of the last evaluated leaves — sums to 1 within 1e-5 (40 iterations
    are ~4 moves per game: no game ends, so the drained set is empty and the priors carry that
    check)."""
    from splendor.nnet import LeafEvaluator, random_net
    net = random_net(2, seed=0)
    default = selfplay_run(lambda e: LeafEvaluator(e, net, 64, use_graph=False))
    f32 = selfplay_run(lambda e: LeafEvaluator(e, net, 64, use_graph=False, precision="f32"))
    assert_same_run(default, f32)
    assert int(default[0]["moves"].sum()) > 64
    a = selfplay_run(lambda e: LeafEvaluator(e, net, 64, use_graph=False, precision="bf16"))
    b = selfplay_run(lambda e: LeafEvaluator(e, net, 64, use_graph=False, precision="bf16"))
    assert_same_run(a, b)
    h, _, ex, events, priors = a
    assert (h["overflow"] == 0).all()
    assert events == {"prunes": 0, "resets": 0, "unexpanded": 0}
    assert int(h["moves"].sum()) > 64
    print(f"bf16 self-play: {int(h['moves'].sum())} moves, {len(ex['pi'])} drained examples")
    np.testing.assert_allclose(ex["pi"].sum(1), 1.0, atol=1e-5)
    np.testing.assert_allclose(priors.sum(1), 1.0, atol=1e-5)
