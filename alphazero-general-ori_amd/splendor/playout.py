"""Leaf evaluation by random playouts: the evaluator of a search player that needs no network.

`PlayoutEvaluator(engine, playouts=4)` has the evaluator signature of splendor.mcts
(`(leaf_state, leaf_mask, leaf_valid) -> (pi, v)`), so `BatchedMCTS(engine, B, args,
evaluator=PlayoutEvaluator(engine))` is the PUCT search with uniform priors whose leaf values
are the mean outcome of `playouts` random games from the leaf: one spl_playout launch per
simulation, nothing else. A leaf is canonical (its mover is seat 0), so the mean outcome in
the leaf's seat order is the frame the network's v has.

Every call draws fresh Philox streams: call number c uses step0 = 256 c mod 2^31 (a playout
has at most 62 n <= 248 moves), so a search repeats exactly from its seed.
"""
from .env import SplendorEngine


class PlayoutEvaluator:
    STREAMS_PER_CALL = 256

    def __init__(self, engine, playouts=1, policy="buy_first", seed=0x5EED, board_base=0):
        if policy not in SplendorEngine.PLAYOUT_POLICIES:
            raise ValueError(f"policy must be one of {sorted(SplendorEngine.PLAYOUT_POLICIES)}, got {policy!r}")
        if not 1 <= int(playouts) <= 64:
            raise ValueError(f"playouts must be in 1..64, got {playouts}")
        self.e = engine
        self.playouts, self.policy = int(playouts), policy
        self.seed, self.board_base = int(seed), int(board_base)
        self.calls = 0

    def __call__(self, leaf_state, leaf_mask, leaf_valid):
        step0 = (self.STREAMS_PER_CALL * self.calls) % (1 << 31)
        self.calls += 1
        out = self.e.playout(leaf_state, active=leaf_valid, policy=self.policy, playouts=self.playouts,
                             seed=self.seed, step0=step0, board_base=self.board_base, pi=True)
        return out["pi"], out["result"]
