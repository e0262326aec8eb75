"""Shared by test_players.py, test_players_gpu.py and test_pit_gpu.py: the players fixtures
(tests/golden/players_*p.npz, make_players_golden.py) and a numpy restatement of the
players' candidate rules (SplendorPlayers.py:105-113 with the mover scored) over the
all-moves definition. Test infrastructure only."""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ST_PLAYER = 8 << 24
CLASS_MIN = 8            # make_players_golden.MIN_PER_CLASS


@functools.lru_cache(maxsize=None)
def fixture(n):
    with np.load(os.path.join(GOLD, f"players_{n}p.npz")) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)
    return d


def greedy_candidates(valid, s0, after):
    """(candidate mask bool[409], m): after[a] = the mover's score after legal move a."""
    v = np.asarray(valid).astype(bool)
    m = int(np.asarray(after)[v].max())
    if m > s0:
        return v & (np.asarray(after) == m), m
    for lo, hi in ((0, 12), (30, 60)):
        c = np.zeros_like(v)
        c[lo:hi] = v[lo:hi]
        if c.any():
            return c, m
    return v, m


def policy_candidates(valid, pi):
    v = np.asarray(valid).astype(bool)
    return v & (pi == pi[v].max())


def pick(cand, u):
    """The k-th candidate in action order, k = floor(u |C|)."""
    c = np.flatnonzero(cand)
    return int(c[int(u * len(c))])


def oracle_after(O, n, board, valid):
    """`after` from the CPU oracle's rules: the all-moves lookahead."""
    out = np.full(409, -1, np.int64)
    for a in np.flatnonzero(valid):
        out[a] = O.score(n, O.make_move(n, board, int(a), 0, True)[0], 0)
    return out


def unpack(words):
    """packed masks [..., 7] (int64 / uint64) -> bool [..., 409]"""
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(*w.shape[:-1], 7 * 64)[..., :409].astype(bool)
