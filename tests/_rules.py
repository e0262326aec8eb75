"""Shared by test_rules.py and test_rules_gpu.py: the reserve-free fixtures
(tests/golden/noreserve_*.npz, make_rules_golden.py) and the rule itself as a function of the
full game's mask. Test infrastructure only."""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RULE_NO_RESERVE = 1
RSV = slice(12, 27)            # reserve a visible card / from a deck
RSV_GIVE = slice(290, 365)     # reserve + give one: not touched by the switch
PASS = 408


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLD, name)) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)
    return d


def no_reserve(mask):
    """f(full mask) (bool / uint8 [..., 409]): bits 12..26 cleared, then pass set iff bits
    0..407 are empty (ENABLE_ACTION_RESERVE = False, SplendorLogicNumba.py:508-510, :263)."""
    m = np.array(mask).astype(bool)
    m[..., RSV] = False
    m[..., PASS] = ~m[..., :PASS].any(-1)
    return m
