"""Leaf evaluation by random playouts: the evaluator of a search player that needs no network.

`PlayoutEvaluator(engine, playouts=4)` has the evaluator signature of splendor.mcts
(`(leaf_state, leaf_mask, leaf_valid) -> (pi, v)`), so `BatchedMCTS(engine, B, args,
evaluator=PlayoutEvaluator(engine))` is the PUCT search with uniform priors whose leaf values
are the mean outcome of `playouts` random games from the leaf: one spl_playout_seq launch per
simulation and one add, nothing else. A leaf is canonical (its mover is seat 0), so the mean
outcome in the leaf's seat order is the frame the network's v has.

Every call draws fresh Philox streams: call number c uses step0 = 256 (c mod 2^23) (a playout
has at most 62 n <= 248 moves), so a search repeats exactly from its seed. The call number
lives in a one-element device tensor that the kernel reads and a stream-ordered add advances,
so a call captured into a graph (SelfPlay.run) draws new streams at every replay. The
evaluator is `indexed`: BatchedMCTS.simulate pairs it with spl_mcts_select_compact and the
playouts run on the listed NN leaves only; called without a list (a plain function wrapped
around it) it runs on the rows flagged in leaf_valid, with the same results. The returned pi
and v are the evaluator's own buffers, one set per batch size, overwritten by the next call
(the rows that did not run keep what they held). `rules` (rule flags, default: the engine's at
the time of each call) are set on the engine around the launch and put back: a reserve-free
search handle on a full-rules engine gets reserve-free playouts and priors.
"""
import torch

from .env import SplendorEngine


class PlayoutEvaluator:
    STREAMS_PER_CALL = 256
    indexed = True

    def __init__(self, engine, playouts=1, policy="buy_first", seed=0x5EED, board_base=0, rules=None):
        if policy not in SplendorEngine.PLAYOUT_POLICIES:
            raise ValueError(f"policy must be one of {sorted(SplendorEngine.PLAYOUT_POLICIES)}, got {policy!r}")
        if not 1 <= int(playouts) <= 64:
            raise ValueError(f"playouts must be in 1..64, got {playouts}")
        self.e = engine
        self.playouts, self.policy = int(playouts), policy
        self.seed, self.board_base = int(seed), int(board_base)
        self.rules = None if rules is None else int(rules)
        self.seq = None                                      # the call number, on the device from the first call
        self._out = {}                                       # batch size -> output buffers (fixed addresses)

    @property
    def calls(self):
        """Calls so far (one small device read after the first call)."""
        return 0 if self.seq is None else int(self.seq.item()) & 0xFFFFFFFF

    def __call__(self, leaf_state, leaf_mask, leaf_valid, index=None, count=None):
        if self.seq is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("PlayoutEvaluator: the first call allocates the call counter and cannot be "
                                   "captured; call once eagerly first (SelfPlay.step does)")
            self.seq = torch.zeros(1, dtype=torch.int32, device=self.e.device)
        listed = index is not None
        own = None if self.rules is None else self.e.rules
        if own is not None:
            self.e.set_rules(flags=self.rules)
        try:
            out = self.e.playout_seq(leaf_state, self.seq, active=None if listed else leaf_valid, index=index,
                                     count=count, policy=self.policy, playouts=self.playouts, seed=self.seed,
                                     board_base=self.board_base, pi=True, out=self._out.get(leaf_state.shape[0]))
        finally:
            if own is not None:
                self.e.set_rules(flags=own)
        self._out[leaf_state.shape[0]] = out
        self.seq += 1                                        # (int32 wraps as the kernel's u32 does)
        return out["pi"], out["result"]
