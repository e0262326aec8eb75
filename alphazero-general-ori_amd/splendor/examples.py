"""Episode-end example pipeline: columnar training examples instead of pickled tuples.

The reference assembles one tuple per example (Coach.py:89-98)

    (board int8[R,7], pi float[409], winner float[n], scdiff int[n], valids bool[409],
     surprise float[n])

and stores each one `zlib.compress(pickle.dumps(x))` (Coach.py:100), the iteration history
pickled whole (`saveTrainExamples`, Coach.py:167-173); training decompresses per sample
(`GenericNNetWrapper.pick_examples`, :326-331) and weighs samples by surprise
(`compute_surprise_weights`, :333-340).

Here an `ExampleSet` keeps the same six fields as columns (device or host tensors, straight
from `SelfPlay.drain()` + `symmetries`), valids bit-packed as the engine's 7 x u64 mask
words. On disk it is a plain `.npz` (numpy arrays only, read back with allow_pickle=False:
nothing is unpickled), optionally deflate-compressed like the reference's zlib level.
`ExampleHistory` is the trainExamplesHistory window (numItersHistory iterations) saved as
one `checkpoint.examples.npz`.

A set comes in two forms. Materialised (`ExampleSet`, file format 1): every symmetry variant
of every recorded position is a stored row, as in the reference. Lazy
(`LazySymmetryExamples`, file format 2): only the recorded positions are stored, 10-18x
fewer rows, and a variant is produced by the engine's gather kernel when a batch is
assembled (a variant is a fixed permutation that depends only on the position's reserved
cards, so nothing about it needs storing). Both present the same row space in the same order.
"""
import os

import numpy as np
import torch

from .env import ACTIONS, MASK_WORDS, pack_mask, unpack_mask

FIELDS = ("board", "pi", "winner", "scdiff", "valids", "surprise")
_FORMAT = 1          # materialised: one stored row per symmetry variant
_FORMAT_LAZY = 2     # lazy: one stored row per recorded position, marker symmetries = "lazy"
_PLAYERS_OF_ROWS = {56: 2, 71: 3, 88: 4}      # observation rows 32 + 10n + n^2


def _file_kind(z, path):
    """Format number of an example file after checking it is one this build reads."""
    fmt = int(z["format"])
    if int(z["actions"]) != ACTIONS or fmt not in (_FORMAT, _FORMAT_LAZY):
        raise ValueError(f"{path}: unsupported example file (format {fmt})")
    if fmt == _FORMAT_LAZY and ("symmetries" not in z.files or str(z["symmetries"]) != "lazy"):
        raise ValueError(f"{path}: format {fmt} without the lazy-symmetries marker")
    return fmt


def symmetry_counts_host(board, n):
    """Number of variants Board.get_symmetries emits per board (SplendorLogicNumba.py:349-395),
    in plain torch on the boards' device: 10 (identity + 3 tiers x 3 card permutations) plus,
    per player, (0, 0, 1, 2)[#reserved cards] reserve permutations, #reserved being the first
    empty reserve slot (_nb_of_reserved_cards, :770-774). board: int8 [E, R, 7] -> uint8 [E].
    The device kernel spl_symmetry_counts states the same rule."""
    board = torch.as_tensor(board)
    rsv = 32 + 4 * n + n * n
    cost = board[:, rsv:rsv + 6 * n:2, :5].to(torch.int64).sum(-1).reshape(-1, n, 3)    # slots' cost rows
    empty = torch.cat([cost == 0, torch.ones_like(cost[:, :, :1], dtype=torch.bool)], dim=2)
    nres = empty.to(torch.int64).argmax(dim=2)                                            # first empty slot
    return (10 + (nres - 1).clamp(min=0).sum(1)).to(torch.uint8)


class ExampleSet:
    """Columnar examples; `valids` is packed [E, 7] int64 (engine mask words)."""

    def __init__(self, board, pi, winner, scdiff, valids, surprise):
        self.board, self.pi, self.winner = board, pi, winner
        self.scdiff, self.valids, self.surprise = scdiff, valids, surprise
        E = board.shape[0]
        for k in FIELDS:
            t = getattr(self, k)
            if t.shape[0] != E:
                raise ValueError(f"field {k}: {t.shape[0]} rows, board has {E}")
        if valids.ndim != 2 or valids.shape[1] != MASK_WORDS:
            raise ValueError(f"valids must be packed [E, {MASK_WORDS}] mask words")

    # ------------------------------------------------------------ construction
    @classmethod
    def from_drain(cls, ex):
        """From SelfPlay.drain() / coach.expand_symmetries output (dict of tensors)."""
        return cls(*(ex[k] for k in FIELDS))

    @classmethod
    def from_tuples(cls, examples):
        """From the reference's list of (board, pi, winner, scdiff, valids, surprise)."""
        if not examples:
            raise ValueError("no examples")
        cols = list(zip(*examples))
        board = torch.from_numpy(np.stack([np.asarray(b, np.int8) for b in cols[0]]))
        pi = torch.from_numpy(np.stack([np.asarray(p, np.float32) for p in cols[1]]))
        winner = torch.from_numpy(np.stack([np.asarray(w, np.float32) for w in cols[2]]))
        scdiff = torch.from_numpy(np.stack([np.asarray(s, np.int32) for s in cols[3]]))
        valids = pack_mask(torch.from_numpy(np.stack([np.asarray(v, bool) for v in cols[4]])))
        surprise = torch.from_numpy(np.stack([np.asarray(s, np.float32) for s in cols[5]]))
        return cls(board, pi, winner, scdiff, valids, surprise)

    @classmethod
    def cat(cls, sets):
        sets = [s for s in sets if len(s)]
        if not sets:
            raise ValueError("no examples")
        dev = sets[0].board.device
        return cls(*(torch.cat([getattr(s, k).to(dev) for s in sets]) for k in FIELDS))

    def __len__(self):
        return int(self.board.shape[0])

    def to(self, device):
        return ExampleSet(*(getattr(self, k).to(device) for k in FIELDS))

    def to_tuples(self):
        """The reference's per-example tuples (Coach.py:91-98), valids unpacked to bool."""
        h = self.to("cpu")
        valids = unpack_mask(h.valids).numpy()
        cols = [h.board.numpy(), h.pi.numpy(), h.winner.numpy(), h.scdiff.numpy(), valids,
                h.surprise.numpy()]
        return [tuple(c[i] for c in cols) for i in range(len(self))]

    # ------------------------------------------------------------ training-side access
    def pick_examples(self, sample_ids):
        """GenericNNetWrapper.pick_examples (:326-331): the six columns of the picked
        samples (a tuple of per-field batches instead of a tuple of tuples)."""
        idx = torch.as_tensor(np.asarray(sample_ids, dtype=np.int64), device=self.board.device)
        out = [getattr(self, k).index_select(0, idx) for k in FIELDS]
        out[4] = unpack_mask(out[4])
        return tuple(out)

    def compute_surprise_weights(self):
        """GenericNNetWrapper.compute_surprise_weights (:333-340), same formula and shape:
        x[-1] is the example's surprise vector [n]; weights = s / s.sum() + 1/len,
        renormalised by the grand total (NumPy's .sum() over every element)."""
        s = self.surprise.detach().cpu().numpy()
        w = s / s.sum() + 1. / len(s)
        return w / w.sum()

    # ------------------------------------------------------------ storage
    def arrays(self):
        h = self.to("cpu")
        return {k: getattr(h, k).numpy() for k in FIELDS}

    def save(self, path, compress=True):
        """Write a .npz (numpy arrays only; `compress` = deflate, the reference's zlib)."""
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        arrs = dict(self.arrays(), format=np.int32(_FORMAT), actions=np.int32(ACTIONS))
        (np.savez_compressed if compress else np.savez)(path, **arrs)

    @classmethod
    def load(cls, path, device="cpu", engine=None):
        """Read a file written by `save`: a format-1 file gives an ExampleSet, a format-2
        (lazy) file a LazySymmetryExamples bound to `engine` (needed for device-resident
        lazy sets; None on the host)."""
        with np.load(path, allow_pickle=False) as z:
            fmt = _file_kind(z, path)
            base = ExampleSet(*(torch.from_numpy(z[k]).to(device) for k in FIELDS))
        return base if fmt == _FORMAT else LazySymmetryExamples(base, engine)


class LazySymmetryExamples:
    """An unexpanded ExampleSet (`base`: one row per recorded position) presenting the row
    space `expand_symmetries` would have stored: every present variant of every position, in
    the reference's order. Rows are produced on demand by the engine's gather kernel.

    counts  uint8 [E]    variants of each position (spl_symmetry_counts; symmetry_counts_host
                         for a host-resident set)
    offsets int64 [E+1]  exclusive prefix sum: rows offsets[i] .. offsets[i+1] belong to i
    len()   the expanded row count (so len // batch_size is the reference's step count)
    n_base  the number of stored positions"""

    def __init__(self, base, engine=None, counts=None):
        if isinstance(base, LazySymmetryExamples):
            base, counts, engine = base.base, base.counts, engine or base.engine
        if base.board.ndim != 3 or base.board.shape[1] not in _PLAYERS_OF_ROWS:
            raise ValueError("lazy examples need boards [E, R, 7]")
        self.base, self.engine = base, engine
        self.n = _PLAYERS_OF_ROWS[base.board.shape[1]]
        if engine is not None and engine.n != self.n:
            raise ValueError(f"boards are {self.n}-player, the engine is {engine.n}-player")
        dev = base.board.device
        if counts is None:
            if dev.type == "cuda":
                counts = self._engine(dev).symmetry_counts(base.board)
            else:
                counts = symmetry_counts_host(base.board, self.n)
        self.counts = counts.to(dev)
        self.offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                  torch.cumsum(self.counts.to(torch.int64), 0)])
        self._ends = self.offsets[1:]
        self._total = int(self.offsets[-1])
        self._err = self._cols = None
        if dev.type == "cuda":           # what every batch hands the kernel, checked once
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
            self._cols = tuple(getattr(base, k).contiguous() for k in ("board", "pi", "valids", "winner", "scdiff"))
            self._engine(dev).check_example_columns(*self._cols)

    def _engine(self, device):
        if self.engine is None:          # no engine given: one of the boards' player count
            from .env import SplendorEngine
            self.engine = SplendorEngine(self.n, device=device)
        return self.engine

    def __len__(self):
        return self._total

    @property
    def n_base(self):
        return len(self.base)

    @property
    def device(self):
        return self.base.board.device

    # ------------------------------------------------------------ construction
    @classmethod
    def cat(cls, sets):
        sets = [s for s in sets if s.n_base]
        if not sets:
            raise ValueError("no examples")
        dev = sets[0].device
        return cls(ExampleSet.cat([s.base for s in sets]), sets[0].engine,
                   counts=torch.cat([s.counts.to(dev) for s in sets]))

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and self.device.type == "cuda":
            device = self.device
        if device == self.device:
            return self
        return LazySymmetryExamples(self.base.to(device), self.engine, counts=self.counts.to(device))

    # ------------------------------------------------------------ rows
    def locate(self, rows, check=True):
        """Expanded row numbers -> (example int64, ordinal int32): the stored position and
        which of its present variants (searchsorted on `offsets`, on the set's device, host
        or HIP). check: raise IndexError for a row outside [0, len) (one host
        synchronisation); batch() skips it and leaves the guard to the kernel."""
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
        if check and rows.numel() and bool(((rows < 0) | (rows >= self._total)).any()):
            raise IndexError(f"row outside [0, {self._total})")
        # position e owns rows offsets[e] .. offsets[e+1]-1: the number of ends <= row. A row
        # past the end lands on e = E and a negative one on a negative ordinal: both are
        # out of range for the kernel's guard
        example = torch.searchsorted(self._ends, rows, right=True)
        ordinal = (rows - self.offsets[example]).to(torch.int32)
        return example, ordinal

    def batch_pairs(self, example, ordinal):
        """(boards f32 [M,R,7], pis [M,409], winner [M,n], scdiff [M,n], valids bool [M,409])
        of the given (position, variant ordinal) pairs, in one kernel launch with no host
        synchronisation. A pair out of range yields a zero row and is reported by
        check_errors()."""
        if self._err is None:
            raise ValueError("batches are assembled on the device: move the set with .to(engine.device)")
        example = torch.as_tensor(example, dtype=torch.int64, device=self.device).contiguous()
        ordinal = torch.as_tensor(ordinal, dtype=torch.int32, device=self.device).contiguous()
        x, pi, valid, winner, scdiff = self.engine.gather_examples(
            *self._cols, example, ordinal, err=self._err, check=False)
        return x, pi, winner, scdiff, valid

    def batch(self, rows):
        """The training batch of expanded rows `rows` (see batch_pairs)."""
        return self.batch_pairs(*self.locate(rows, check=False))

    def check_errors(self):
        """Raise if any batch since the last call asked for a row or variant out of range
        (synchronises; the kernel only ORs a flag so assembling batches never waits)."""
        if self._err is not None and int(self._err.item()):
            self._err.zero_()
            raise IndexError("lazy examples: a batch asked for a row or variant out of range")

    def materialize(self):
        """The ExampleSet expand_symmetries would have stored (on the engine's device)."""
        from .coach import expand_symmetries
        eng = self._engine(self.device if self.device.type == "cuda" else "cuda")
        b = self.base.to(eng.device)
        return ExampleSet.from_drain(expand_symmetries(eng, {k: getattr(b, k).contiguous() for k in FIELDS}))

    # ------------------------------------------------------------ storage
    def save(self, path, compress=True):
        """Write the base columns only, marked format 2 / symmetries = "lazy"."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        arrs = dict(self.base.arrays(), format=np.int32(_FORMAT_LAZY), actions=np.int32(ACTIONS),
                    symmetries=np.array("lazy"))
        (np.savez_compressed if compress else np.savez)(path, **arrs)

    @classmethod
    def load(cls, path, device="cpu", engine=None):
        out = ExampleSet.load(path, device=device, engine=engine)
        if not isinstance(out, cls):
            raise ValueError(f"{path}: not a lazy-symmetries example file")
        return out


class ExampleHistory:
    """Coach.trainExamplesHistory: one ExampleSet per iteration, at most `max_iters`
    (args.numItersHistory, Coach.py:134-135), saved/loaded as checkpoint.examples.npz
    (saveTrainExamples / loadTrainExamples, Coach.py:167-190)."""

    FILE = "checkpoint.examples.npz"

    def __init__(self, max_iters=None):
        self.max_iters = max_iters
        self.iters = []

    def append(self, exset):
        self.iters.append(exset)
        if self.max_iters is not None and len(self.iters) > self.max_iters:
            self.iters.pop(0)

    def __len__(self):
        return sum(len(s) for s in self.iters)

    def is_lazy(self):
        """True when the window holds lazy sets (a window holds one kind only)."""
        kinds = {isinstance(s, LazySymmetryExamples) for s in self.iters}
        if len(kinds) > 1:
            raise ValueError("the example history mixes lazy and materialised sets")
        return kinds == {True}

    def merged(self):
        if self.is_lazy():
            return LazySymmetryExamples.cat(self.iters)
        return ExampleSet.cat(self.iters)

    def save(self, folder, compress=True):
        """One .npz for the window. A lazy window stores its base rows only (`sizes` then
        counts stored positions per iteration) with format 2 and symmetries = "lazy"."""
        os.makedirs(folder, exist_ok=True)
        lazy = self.is_lazy()
        sets = [s.base for s in self.iters] if lazy else self.iters
        sizes = np.array([len(s) for s in sets], np.int64)
        merged = ExampleSet.cat(sets).arrays() if len(sizes) and sizes.sum() else {}
        head = dict(format=np.int32(_FORMAT_LAZY), symmetries=np.array("lazy")) if lazy else \
            dict(format=np.int32(_FORMAT))
        path = os.path.join(folder, self.FILE)
        (np.savez_compressed if compress else np.savez)(
            path, actions=np.int32(ACTIONS), sizes=sizes, **head, **merged)
        return path

    @classmethod
    def load(cls, folder, max_iters=None, device="cpu", engine=None):
        """Read a window: format 1 gives ExampleSets as before, format 2 gives
        LazySymmetryExamples bound to `engine` (needed when `device` is a HIP device)."""
        h = cls(max_iters)
        path = os.path.join(folder, cls.FILE)
        with np.load(path, allow_pickle=False) as z:
            fmt = _file_kind(z, path)
            sizes = z["sizes"]
            if not len(sizes) or not sizes.sum():
                return h
            cols = {k: torch.from_numpy(z[k]).to(device) for k in FIELDS}
        off = 0
        for n in sizes.tolist():
            part = ExampleSet(*(cols[k][off:off + n] for k in FIELDS))
            h.append(part if fmt == _FORMAT else LazySymmetryExamples(part, engine))
            off += n
        return h
