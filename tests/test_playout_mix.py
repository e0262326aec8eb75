"""CPU checks of spl_playout_mix's boundary: the header declares it, the built library exports
it, the ctypes binding lists it, every bad argument is rejected before any launch (no device is
touched: the calls run on a machine without a GPU), the mixed evaluator checks its arguments
without an engine, and a Coach without rollout_mix builds none."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splendor_amd.h")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsplendor_amd.so not built")


def test_header_declares_playout_mix():
    src = open(HEADER).read()
    assert re.search(r"^\s*int\s+spl_playout_mix\s*\(", src, flags=re.M)
    assert re.search(r"^#define\s+SPL_ABI_VERSION\s+11\s*$", src, flags=re.M)     # additive: no bump


@needs_lib
def test_library_exports_playout_mix():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "spl_playout_mix") and hasattr(lib, "spl_playout_seq") and hasattr(lib, "spl_playout")
    assert lib.spl_abi_version() == 11


@needs_lib
def test_binding_lists_playout_mix():
    from splendor import _lib
    assert "spl_playout_mix" in _lib.exported_symbols()
    args, res = _lib._SIGS["spl_playout_mix"]
    assert len(args) == 16 and res is ctypes.c_int
    assert _lib.ABI_VERSION == 11
    from splendor.env import SplendorEngine
    assert callable(SplendorEngine.playout_mix)


@needs_lib
def test_playout_mix_argument_validation():
    """SPL_EINVAL for every argument the header rules out, and B == 0 as a no-op, all before
    any launch (the pointers are dummies that are never dereferenced)."""
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    f = lib.spl_playout_mix
    f.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, vp]
    f.restype = ci
    lib.spl_ctx_destroy.argtypes = [vp]
    h = vp()
    assert lib.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    d = vp(1)

    def call(ctx=h, B=0, state=d, active=None, index=None, count=None, policy=1, playouts=1, max_steps=124,
             seq=d, lam=d, v=d):
        return f(ctx, B, state, active, index, count, policy, playouts, max_steps, 0x5EED, seq, 0, lam, v, None,
                 None)

    assert call() == 0                                        # B == 0: nothing launched
    assert call(policy=0, playouts=64, max_steps=256) == 0
    assert call(active=d) == 0
    assert call(index=d, count=d) == 0
    assert call(max_steps=1) == 0
    assert call(ctx=None) == -1
    assert call(state=None) == -1
    assert call(seq=None) == -1
    assert call(lam=None) == -1
    assert call(v=None) == -1
    assert call(B=4, lam=None) == -1
    assert call(B=4, v=None) == -1
    assert call(active=d, index=d, count=d) == -1             # flags together with a list
    assert call(index=d) == -1                                # half a list
    assert call(count=d) == -1
    assert call(active=d, index=d) == -1
    assert call(active=d, count=d) == -1
    for max_steps in (0, 257):
        assert call(max_steps=max_steps) == -1
    for policy in (-1, 2):
        assert call(policy=policy) == -1
    for playouts in (0, 65):
        assert call(playouts=playouts) == -1
    assert call(B=-1) == -1
    lib.spl_ctx_destroy(h)


class ListNetwork:
    """What MixedEvaluator asks of its network before the first call: `indexed`."""
    indexed = True


def test_mixed_evaluator_checks_its_arguments_without_a_device():
    from splendor.playout import MixedEvaluator, PlayoutEvaluator
    net = ListNetwork()
    ev = MixedEvaluator(None, net, playouts=4, policy="uniform", lam=0.25, seed=3, board_base=7)
    assert ev.calls == 0 and ev.indexed is True and not getattr(ev, "staged", False)
    assert (ev.playouts, ev.policy, ev.lam, ev.seed, ev.board_base) == (4, "uniform", 0.25, 3, 7)
    assert ev.network is net and ev.unfinished == 0
    d = MixedEvaluator(None, net)
    assert (d.playouts, d.policy, d.lam, d.seed, d.board_base, d.rules) == (4, "buy_first", 0.5, 0x5EED, 0, None)
    assert d.STREAMS_PER_CALL == PlayoutEvaluator.STREAMS_PER_CALL == 256
    with pytest.raises(ValueError):
        MixedEvaluator(None, net, policy="greedy")
    for playouts in (0, 65):
        with pytest.raises(ValueError):
            MixedEvaluator(None, net, playouts=playouts)
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            MixedEvaluator(None, net, lam=lam)
        with pytest.raises(ValueError):
            ev.lam = lam
    assert ev.lam == 0.25                                     # a rejected value changes nothing
    for lam in (0.0, 1.0):
        ev.lam = lam                                          # (no device scalar yet: the host value only)
        assert ev.lam == lam
    for bad in (None, object(), lambda s, m, v: None, type("Eager", (), {"indexed": False})()):
        with pytest.raises(ValueError):
            MixedEvaluator(None, bad)
        with pytest.raises(ValueError):
            ev.set_network(bad)
    assert ev.network is net
    other = ListNetwork()
    ev.set_network(other)
    assert ev.network is other and ev.calls == 0


def test_coach_without_rollout_mix_constructs_no_mixed_evaluator(monkeypatch):
    """Coach.__init__ and the lambda schedule run on a stand-in self-play handle (no engine): no
    MixedEvaluator is built when rollout_mix is absent or 0, and learn()'s schedule is the
    issue's (a float for every iteration, a sequence by iteration, 0 past its end)."""
    from splendor import coach as coach_mod

    def no_mixed(*a, **k):
        raise AssertionError("a MixedEvaluator was built without rollout_mix")

    class Handle:
        rules = 0

        def __init__(self, engine, B, args, evaluator=None, **kw):
            self.evaluator = evaluator

        def reset(self):
            pass

    class Game:
        engine = None

    monkeypatch.setattr(coach_mod, "MixedEvaluator", no_mixed)
    monkeypatch.setattr(coach_mod, "SelfPlay", Handle)
    monkeypatch.setattr(coach_mod, "evaluator_for", lambda *a, **k: ListNetwork())
    for args in ({}, {"rollout_mix": 0}, {"rollout_mix": 0.0}, {"rollout_mix": None}, {"rollout_mix": []}):
        c = coach_mod.Coach(Game(), None, dict(args, numItersHistory=2), batch=4)
        assert c._mixed_ev == {} and isinstance(c.sp.evaluator, ListNetwork)
        assert [c._mix_lambda(i) for i in (1, 2, 3)] == [0.0, 0.0, 0.0]
    c = coach_mod.Coach(Game(), None, {"rollout_mix": 0.5, "numItersHistory": 2}, batch=4)
    assert c._mixed_ev == {} and [c._mix_lambda(i) for i in (1, 2, 9)] == [0.5, 0.5, 0.5]
    c = coach_mod.Coach(Game(), None, {"rollout_mix": (0.5, 0, 0.25), "numItersHistory": 2}, batch=4)
    assert c._mixed_ev == {} and [c._mix_lambda(i) for i in (1, 2, 3, 4)] == [0.5, 0.0, 0.25, 0.0]
    with pytest.raises(AssertionError):
        c.use_mixed_selfplay(0.5)
