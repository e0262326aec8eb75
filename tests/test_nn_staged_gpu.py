"""The staged leaf buffer on the GPU: spl_nn_stage_leaves (the mask kernel filling the buffer
from caller-supplied boards) followed by spl_nn_forward_staged must give, on every listed row,
exactly the bits of spl_nn_forward_indexed on the same list, in all three precision modes, and
leave every other row alone; the buffer's list (total, rows, masks) and the masks written by
tree row are checked directly. One buffer per player count is reused by all validity patterns
in turn, so every pattern but the first meets the previous one's stale entries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 200                      # four 64-tree segments, the last of 8 trees; tiles straddle segments
PATTERNS = ("random", "empty_and_full", "all", "none", "total32", "total33")


def _valid(pattern, n_rows, rng):
    v = np.zeros(n_rows, np.uint8)
    if pattern == "random":
        v[:] = rng.random(n_rows) < 0.7
    elif pattern == "empty_and_full":
        v[:] = rng.random(n_rows) < 0.7
        v[0:64] = 1
        v[64:128] = 0
    elif pattern == "all":
        v[:] = 1
    elif pattern in ("total32", "total33"):
        v[rng.choice(n_rows, int(pattern[5:]), replace=False)] = 1
    return v


@functools.lru_cache(maxsize=None)
def _setup(n, n_rows):
    """Engine, canonical boards of random games, their masks, the packed network per precision and
    the (zero-filled once) staged buffer."""
    from splendor.env import RolloutBatch, SplendorEngine
    from splendor.nnet import FusedNet, new_stage, random_net
    eng = SplendorEngine(n, device="cuda:0")
    rb = RolloutBatch(eng, n_rows, seed=100 + n)
    rb.run(30)
    boards = eng.canonical(rb.state, rb.player).contiguous()
    masks = eng.valid_moves(boards).contiguous()
    net = random_net(n, seed=7)
    fused = {p: FusedNet(net, n, "cuda:0", precision=p) for p in ("f32", "bf16x2", "bf16")}
    return eng, boards, masks, fused, new_stage(n, n_rows, "cuda:0")


def _segment_list(valid):
    n_rows = len(valid)
    nseg = (n_rows + 63) // 64
    index = np.zeros(n_rows, np.int32)
    count = np.zeros(nseg, np.int32)
    for j in range(nseg):
        r = np.nonzero(valid[64 * j:64 * j + 64])[0].astype(np.int32) + 64 * j
        index[64 * j:64 * j + len(r)] = r
        count[j] = len(r)
    return index, count


def _check(n, n_rows, valid_np, precisions):
    from splendor import _lib
    from splendor.env import _ptr
    eng, boards, masks, fused, stage = _setup(n, n_rows)
    dev = boards.device
    valid = torch.from_numpy(valid_np).to(dev)
    rows_np = np.nonzero(valid_np)[0]
    rows = torch.from_numpy(rows_np).to(dev)
    other = torch.from_numpy(valid_np == 0).to(dev)
    by_tree = torch.full((n_rows, 7), -5, dtype=torch.int64, device=dev)
    _lib.check(eng.L.spl_nn_stage_leaves(eng.ctx, n_rows, _ptr(boards), _ptr(valid), _ptr(by_tree), _ptr(stage),
                                         eng._s()), "spl_nn_stage_leaves")
    # masks by tree row: the rule's mask on listed rows (the engine's spl_valid_moves, the mask the
    # search's mask kernel computes for a canonical leaf), the sentinel elsewhere
    assert torch.equal(by_tree[rows], masks[rows])
    assert bool((by_tree[other] == -5).all())
    # the buffer's list: total, rows (segments in order, trees ascending) and masks in list order
    total = int(stage[:4].view(torch.int32).item())
    assert total == len(rows_np)
    m_off = (16 + 4 * n_rows + 15) // 16 * 16
    assert torch.equal(stage[16:16 + 4 * total].view(torch.int32), rows.to(torch.int32))
    assert torch.equal(stage[m_off:m_off + 56 * total].view(torch.int64).view(-1, 7), masks[rows])
    index_np, count_np = _segment_list(valid_np)
    index, count = torch.from_numpy(index_np).to(dev), torch.from_numpy(count_np).to(dev)
    for p in precisions:
        f = fused[p]
        pi = torch.full((n_rows, 409), -7.0, device=dev)
        v = torch.full((n_rows, n), -7.0, device=dev)
        f(boards, by_tree, pi, v, stage=stage)
        pi_ref = torch.full((n_rows, 409), -7.0, device=dev)
        v_ref = torch.full((n_rows, n), -7.0, device=dev)
        _lib.check(_lib.lib().spl_nn_forward_mode(n, n_rows, _ptr(boards), _ptr(by_tree), _ptr(index), _ptr(count),
                                                  _ptr(f.w), _ptr(pi_ref), _ptr(v_ref), f.mode,
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "spl_nn_forward_mode")
        assert torch.equal(pi[rows], pi_ref[rows]) and torch.equal(v[rows], v_ref[rows]), p
        assert bool((pi[other] == -7.0).all()) and bool((v[other] == -7.0).all()), p
        if total:
            assert bool((pi_ref[rows] != -7.0).any())          # (the reference did run)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", (2, 3, 4))
def test_staged_equals_indexed(n, pattern):
    """spl_nn_forward_indexed is spl_nn_forward_mode(SPL_NN_F32) with a list; the reduced modes
    go through spl_nn_forward_mode too, so one entry point gives all three references."""
    rng = np.random.default_rng(1000 * n + PATTERNS.index(pattern))
    _check(n, B, _valid(pattern, B, rng), ("f32", "bf16x2", "bf16"))


def test_staged_prefix_beyond_one_pass():
    """B = 64 x 513 + 5: more than 512 segments (the prefix sum over leaf_valid takes a second
    pass in the last segments) and a partial last segment."""
    n_rows = 64 * 513 + 5
    rng = np.random.default_rng(77)
    _check(2, n_rows, (rng.random(n_rows) < 0.7).astype(np.uint8), ("f32",))
