"""Reduced-precision modes of the fused network kernel, host side (no GPU): the float64 host
reference that defines the modes (splendor.nnet.reduced_forward) on the nnet_{n}p fixture with
test_nnet.py's closed-form weights, the precision argument's plumbing, and the argument checks
of spl_nn_forward_mode (rejected before any launch, so no device is needed)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from test_nnet import deterministic_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")

# max |pi - pi_f32|, max |v - v_f32| of each reduced mode on the fixture (float64 emulation of
# the mode definition; equal for n = 2, 3, 4 to two digits)
FIXTURE_DISTANCE = {"bf16": (8.3e-6, 9.4e-4), "bf16x2": (3.2e-8, 4.0e-6)}

_cache = {}


def fixture_forward(n, precision):
    """(pi, v) float64 numpy of reduced_forward on the fixture, computed once per (n, mode)."""
    from splendor.nnet import FoldedNet, SplendorNNet, reduced_forward
    if ("net", n) not in _cache:
        with np.load(os.path.join(GOLD, f"nnet_{n}p.npz")) as z:
            g = {k: z[k] for k in z.files}
        net = SplendorNNet(n)
        net.load_state_dict(deterministic_weights(net.state_dict()))
        _cache[("net", n)] = (g, FoldedNet(net.eval()))
    g, fold = _cache[("net", n)]
    if (n, precision) not in _cache:
        pi, v = reduced_forward(fold, torch.from_numpy(g["boards"].astype(np.float32)),
                                torch.from_numpy(g["valid"]), precision)
        assert pi.dtype == torch.float64 and v.dtype == torch.float64
        _cache[(n, precision)] = (pi.numpy(), v.numpy())
    return _cache[(n, precision)]


@pytest.mark.parametrize("n", (2, 3, 4))
def test_reduced_forward_f32_is_the_folded_net(n):
    """The "f32" definition (six part products) is FoldedNet within test_nnet.py's fp32
    tolerances: 1e-6 absolute + 1e-4 relative on pi, 1e-5 on v."""
    pi, v = fixture_forward(n, "f32")
    g, fold = _cache[("net", n)]
    with torch.no_grad():
        pr, vr = fold(torch.from_numpy(g["boards"].astype(np.float32)), torch.from_numpy(g["valid"]))
    np.testing.assert_allclose(pi, pr.numpy(), atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(v, vr.numpy(), atol=1e-5)
    np.testing.assert_allclose(pi, np.exp(g["log_pi"].astype(np.float64)) * g["valid"], atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(v, g["v"], atol=1e-5)


@pytest.mark.parametrize("n", (2, 3, 4))
def test_reduced_mode_fixture_distances(n):
    """Each reduced mode's distance from "f32" on the fixture is within a factor of 4 of the
    tabulated value, and bf16x2's is at least 16 times smaller than bf16's."""
    pi0, v0 = fixture_forward(n, "f32")
    d = {}
    for mode, (tpi, tv) in FIXTURE_DISTANCE.items():
        pi, v = fixture_forward(n, mode)
        dpi, dv = np.abs(pi - pi0).max(), np.abs(v - v0).max()
        print(f"n={n} {mode}: max|dpi|={dpi:.3e} max|dv|={dv:.3e}")
        assert tpi / 4 <= dpi <= 4 * tpi
        assert tv / 4 <= dv <= 4 * tv
        np.testing.assert_allclose(pi.sum(1), 1.0, atol=1e-12)
        d[mode] = (dpi, dv)
    assert 16 * d["bf16x2"][0] <= d["bf16"][0] and 16 * d["bf16x2"][1] <= d["bf16"][1]


def test_unknown_precision_names_raise():
    from splendor.nnet import FoldedNet, FusedNet, LeafEvaluator, SplendorNNet, precision_mode, reduced_forward
    from splendor.search import evaluator_for
    assert [precision_mode(p) for p in ("f32", "bf16x2", "bf16")] == [0, 1, 2]
    net = SplendorNNet(2)
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError):
            precision_mode(bad)
        with pytest.raises(ValueError):                        # (before anything touches a device)
            FusedNet(net, 2, "cpu", precision=bad)
        with pytest.raises(ValueError):
            LeafEvaluator(types.SimpleNamespace(n=2, device=torch.device("cpu"), rows=56), net, 4, precision=bad)
    with pytest.raises(ValueError):
        reduced_forward(FoldedNet(net), torch.zeros((1, 56, 7)), torch.ones((1, 409), dtype=torch.bool), "half")
    with pytest.raises(ValueError):
        evaluator_for(None, object(), 1, precision="half")
    # a reduced mode is the fused kernel's: the FoldedNet path has none
    with pytest.raises(ValueError):
        LeafEvaluator(types.SimpleNamespace(n=2, device=torch.device("cpu"), rows=56), net, 4, fused=False,
                      precision="bf16")


def test_nn_precision_argument_plumbing(monkeypatch):
    """nn_precision is read from a dict and from an attribute object, defaults to "f32", and
    reaches evaluator_for from Coach and (one value, or one per player) from BatchedArena."""
    from splendor import arena, coach, search
    from splendor.search import nn_precision_arg
    assert nn_precision_arg({}) == "f32"
    assert nn_precision_arg(types.SimpleNamespace()) == "f32"
    assert nn_precision_arg({"nn_precision": "bf16"}) == "bf16"
    assert nn_precision_arg(types.SimpleNamespace(nn_precision="bf16x2")) == "bf16x2"
    assert arena.arena_precisions({}) == ("f32", "f32")
    assert arena.arena_precisions({"nn_precision": "bf16"}) == ("bf16", "bf16")
    assert arena.arena_precisions(types.SimpleNamespace(nn_precision=("bf16", "f32"))) == ("bf16", "f32")
    assert arena.arena_precisions({"nn_precision": ["f32", "bf16x2"]}) == ("f32", "bf16x2")
    with pytest.raises(ValueError):
        arena.arena_precisions({"nn_precision": ("f32", "bf16", "bf16")})
    # evaluator_for: no precision means "f32"; a reference-style nnet.predict takes any valid mode
    assert isinstance(search.evaluator_for(None, object(), 1), search.PredictEvaluator)
    assert isinstance(search.evaluator_for(None, object(), 1, precision="bf16"), search.PredictEvaluator)
    # Coach / BatchedArena hand args.nn_precision to evaluator_for
    seen = []

    class Stop(Exception):
        pass

    def spy(engine, nnet, batch=1, precision=None):
        seen.append(precision)
        if len(seen) % 2 == 0 or engine == "coach":
            raise Stop
        return None
    monkeypatch.setattr(coach, "evaluator_for", spy)
    monkeypatch.setattr(arena, "evaluator_for", spy)
    game = types.SimpleNamespace(engine="coach")
    for args, want in (({"numEps": 1}, "f32"), ({"numEps": 1, "nn_precision": "bf16"}, "bf16"),
                       (types.SimpleNamespace(numEps=1, nn_precision="bf16x2"), "bf16x2")):
        seen.clear()
        with pytest.raises(Stop):
            coach.Coach(game, None, args)
        assert seen == [want]
    game = types.SimpleNamespace(engine=types.SimpleNamespace(n=2))
    for args, want in (({}, ["f32", "f32"]), ({"nn_precision": "bf16"}, ["bf16", "bf16"]),
                       (types.SimpleNamespace(nn_precision=("bf16", "f32")), ["bf16", "f32"])):
        seen.clear()
        with pytest.raises(Stop):
            arena.BatchedArena(game, None, None, args, batch=4)
        assert seen == want


def test_no_environment_variable_selects_a_mode():
    """The mode comes from the precision argument alone (the benchmark's kernel cannot be changed
    from outside): the package's network module reads no environment variable."""
    import splendor.nnet as m
    src = open(m.__file__).read()
    assert "environ" not in src and "getenv" not in src


@pytest.mark.skipif(not os.path.exists(LIB), reason="libsplendor_amd.so not built")
def test_forward_mode_argument_validation():
    """spl_nn_forward_mode: precision outside 0 .. 2 and exactly one of leaf_index / leaf_count
    NULL are SPL_EINVAL before any launch; B == 0 returns 0 in every mode."""
    from splendor import _lib
    L = _lib.lib()
    assert L.spl_abi_version() == 11
    vp = ctypes.c_void_p
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = vp((base + 63) // 64 * 64)                                      # any aligned non-NULL pointer

    def call(B, index, count, precision):
        return L.spl_nn_forward_mode(2, B, p, p, index, count, p, p, p, precision, None)
    for bad in (3, -1):
        assert call(32, None, None, bad) == _lib.EINVAL
        assert call(32, p, p, bad) == _lib.EINVAL
        assert call(0, None, None, bad) == _lib.EINVAL
    for mode in (0, 1, 2):
        assert call(32, p, None, mode) == _lib.EINVAL
        assert call(32, None, p, mode) == _lib.EINVAL
        assert call(0, None, None, mode) == 0
        assert call(0, p, p, mode) == 0
        assert L.spl_nn_forward_mode(5, 32, p, p, None, None, p, p, p, mode, None) == _lib.EINVAL
        assert L.spl_nn_forward_mode(2, 32, None, p, None, None, p, p, p, mode, None) == _lib.EINVAL
