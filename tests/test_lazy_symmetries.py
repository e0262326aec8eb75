"""Lazy symmetry expansion, host side: the count rule against the reference-executed
fixtures (tests/golden/sym_*p.npz: 40 positions each, off[i]..off[i+1] the rows of position
i), row -> (position, variant) lookup, the two storage formats, and the argument checks of
the two C entry points (no device is touched: every call returns before a launch)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from splendor.env import pack_mask  # noqa: E402
from splendor.examples import (ExampleHistory, ExampleSet, LazySymmetryExamples,  # noqa: E402
                               symmetry_counts_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "alphazero-general-ori_amd", "libsplendor_amd.so")


def fixture(n):
    with np.load(os.path.join(GOLD, f"sym_{n}p.npz")) as z:
        return {k: z[k] for k in z.files}


def base_set(d, n):
    """The fixture's 40 source positions as an unexpanded host ExampleSet (winner / scdiff /
    surprise: distinct values per position)."""
    E = len(d["src"])
    g = torch.Generator().manual_seed(100 + n)
    return ExampleSet(torch.from_numpy(d["src"]), torch.from_numpy(d["src_pi"]),
                      torch.rand((E, n), generator=g) * 2 - 1,
                      torch.randint(-15, 16, (E, n), generator=g, dtype=torch.int32),
                      pack_mask(torch.from_numpy(d["src_valids"]).bool()),
                      torch.rand((E, n), generator=g))


@pytest.mark.parametrize("n", (2, 3, 4))
def test_host_counts_match_reference(n):
    d = fixture(n)
    counts = symmetry_counts_host(torch.from_numpy(d["src"]), n)
    assert counts.dtype == torch.uint8
    np.testing.assert_array_equal(counts.numpy(), np.diff(d["off"]))


@pytest.mark.parametrize("n", (2, 3, 4))
def test_locate(n):
    d = fixture(n)
    off = d["off"]
    lz = LazySymmetryExamples(base_set(d, n))
    total = int(off[-1])
    assert len(lz) == total == len(d["state"]) and lz.n_base == 40
    assert lz.offsets.dtype == torch.int64 and lz.offsets.tolist() == off.tolist()
    ex, od = lz.locate(torch.from_numpy(off[:-1]))                  # first row of every position
    assert ex.tolist() == list(range(40)) and od.tolist() == [0] * 40
    ex, od = lz.locate(torch.from_numpy(off[1:] - 1))               # last row of every position
    assert ex.tolist() == list(range(40)) and od.tolist() == (np.diff(off) - 1).tolist()
    ex, od = lz.locate(torch.arange(total))                         # the fixture's row order
    want_ex = np.repeat(np.arange(40), np.diff(off))
    np.testing.assert_array_equal(ex.numpy(), want_ex)
    np.testing.assert_array_equal(od.numpy(), np.arange(total) - off[want_ex])
    assert ex.dtype == torch.int64 and od.dtype == torch.int32
    for bad in ([total], [-1], [0, total + 5], [3, -2]):
        with pytest.raises(IndexError):
            lz.locate(torch.tensor(bad))


def test_lazy_history_roundtrip(tmp_path):
    """A lazy window saves its base rows only (format 2, marker "lazy") and loads without
    pickle as lazy sets with the same rows, counts and iteration split."""
    d2 = fixture(2)
    full = base_set(d2, 2)
    a = LazySymmetryExamples(ExampleSet(*(getattr(full, k)[:25] for k in
                                          ("board", "pi", "winner", "scdiff", "valids", "surprise"))))
    b = LazySymmetryExamples(ExampleSet(*(getattr(full, k)[25:] for k in
                                          ("board", "pi", "winner", "scdiff", "valids", "surprise"))))
    h = ExampleHistory(max_iters=3)
    h.append(a)
    h.append(b)
    assert len(h) == 539 and isinstance(h.merged(), LazySymmetryExamples) and h.merged().n_base == 40
    path = h.save(str(tmp_path))
    with np.load(path, allow_pickle=False) as z:
        assert int(z["format"]) == 2 and str(z["symmetries"]) == "lazy"
        assert z["board"].shape == (40, 56, 7) and z["pi"].shape == (40, 409)
        assert z["sizes"].tolist() == [25, 15]
        assert all(z[k].dtype != object for k in z.files)
    back = ExampleHistory.load(str(tmp_path), max_iters=3)
    assert [type(s) for s in back.iters] == [LazySymmetryExamples] * 2
    assert [s.n_base for s in back.iters] == [25, 15] and len(back) == 539
    for s, t in zip(back.iters, (a, b)):
        assert torch.equal(s.counts, t.counts) and torch.equal(s.offsets, t.offsets)
        for k in ("board", "pi", "winner", "scdiff", "valids", "surprise"):
            assert torch.equal(getattr(s.base, k), getattr(t.base, k)), k
    # one set on its own
    one = os.path.join(str(tmp_path), "one.npz")
    a.save(one)
    la = LazySymmetryExamples.load(one)
    assert la.n_base == 25 and len(la) == len(a) and torch.equal(la.base.pi, a.base.pi)
    assert isinstance(ExampleSet.load(one), LazySymmetryExamples)
    m = LazySymmetryExamples.cat([a, b])
    assert torch.equal(m.counts, torch.cat([a.counts, b.counts])) and len(m) == 539


def test_format1_history_loads_as_before(tmp_path):
    """A materialised window is written and read exactly as before: format 1, every row
    stored, plain ExampleSets back."""
    d = fixture(2)
    n_rows = len(d["state"])
    g = torch.Generator().manual_seed(7)
    es = ExampleSet(torch.from_numpy(d["state"]), torch.from_numpy(d["pi"]), torch.rand((n_rows, 2), generator=g),
                    torch.randint(-15, 16, (n_rows, 2), generator=g, dtype=torch.int32),
                    pack_mask(torch.from_numpy(d["valids"]).bool()), torch.rand((n_rows, 2), generator=g))
    h = ExampleHistory()
    h.append(es)
    path = h.save(str(tmp_path))
    with np.load(path, allow_pickle=False) as z:
        assert int(z["format"]) == 1 and "symmetries" not in z.files
        assert sorted(z.files) == sorted(["format", "actions", "sizes", "board", "pi", "winner", "scdiff", "valids",
                                          "surprise"])
        assert z["sizes"].tolist() == [n_rows]
    back = ExampleHistory.load(str(tmp_path))
    assert [type(s) for s in back.iters] == [ExampleSet] and not back.is_lazy()
    for k in ("board", "pi", "winner", "scdiff", "valids", "surprise"):
        assert torch.equal(getattr(back.iters[0], k), getattr(es, k)), k
    single = os.path.join(str(tmp_path), "set.npz")
    es.save(single)
    assert type(ExampleSet.load(single)) is ExampleSet


def test_entry_points_check_arguments():
    """spl_symmetry_counts / spl_gather_examples: SPL_EINVAL for a NULL context, negative
    sizes or a NULL required pointer, 0 without a launch for E == 0 or M == 0; the ABI
    version is unchanged."""
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.spl_abi_version() == 11
    counts, gather = lib.spl_symmetry_counts, lib.spl_gather_examples
    counts.argtypes = [vp, ci, vp, vp, vp]
    gather.argtypes = [vp, ci, ci] + [vp] * 14
    h = vp()
    lib.spl_ctx_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    assert lib.spl_ctx_create(2, 10, ctypes.byref(h)) == 0
    p = vp(16)                                   # never dereferenced: every call returns before a launch
    assert counts(None, 4, p, p, None) == -1
    assert counts(h, -1, p, p, None) == -1
    assert counts(h, 4, None, p, None) == -1
    assert counts(h, 4, p, None, None) == -1
    assert counts(h, 0, None, None, None) == 0
    ptrs = [p] * 12                              # state .. out_scdiff (err and the stream may be NULL)
    assert gather(None, 4, 4, *ptrs, None, None) == -1
    assert gather(h, -1, 4, *ptrs, None, None) == -1
    assert gather(h, 4, -1, *ptrs, None, None) == -1
    for k in range(12):
        args = list(ptrs)
        args[k] = None
        assert gather(h, 4, 4, *args, None, None) == -1, k
    assert gather(h, 0, 4, *([None] * 12), None, None) == 0
    assert gather(h, 4, 0, *([None] * 12), None, None) == 0
    lib.spl_ctx_destroy.argtypes = [vp]
    lib.spl_ctx_destroy(h)
    from splendor import _lib
    assert {"spl_symmetry_counts", "spl_gather_examples"} <= set(_lib.exported_symbols())
    assert _lib.ABI_VERSION == 11 and _lib.ERR_BAD_INDEX == 2
