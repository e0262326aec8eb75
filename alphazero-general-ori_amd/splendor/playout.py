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

`MixedEvaluator(engine, network, playouts=4, lam=0.5)` keeps the network's priors and mixes
the two values, (1 - lam) v_network + lam v_playout (spl_playout_mix), on the same list.
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


class MixedEvaluator(PlayoutEvaluator):
    """AlphaGo's mixed leaf evaluation: the network's priors, and the leaf value
    (1 - lam) v_network + lam v_playout with v_playout the mean of `playouts` random games.

    `network` is a fused splendor.nnet.LeafEvaluator (anything `indexed`); `set_network`
    replaces it and keeps the call counter. A call runs the network on the leaf list, then one
    spl_playout_mix launch on the same list that blends the playout means into the network's v
    buffer, then the stream-ordered advance of the call counter: (the network's pi, the mixed
    v). The evaluator is `indexed` and not `staged`, so BatchedMCTS.simulate hands it the
    compacted list; called without a list it runs the network on every row and the playouts on
    the rows flagged in leaf_valid, with the same results on those rows. Rules, policies,
    playouts, seed, board_base and the call counter are PlayoutEvaluator's: at lam = 1 the
    values are those of a PlayoutEvaluator with the same arguments and call number. `lam` lives
    in a one-element device tensor that the kernel reads: assigning it is a stream-ordered fill
    that reaches captured launches, so changing it never drops a graph. At lam = 0 the playout
    launch leaves at once and the search is the network's, bit for bit."""

    def __init__(self, engine, network, playouts=4, policy="buy_first", lam=0.5, seed=0x5EED, board_base=0,
                 rules=None):
        super().__init__(engine, playouts, policy, seed=seed, board_base=board_base, rules=rules)
        self._lam = self._check_lam(lam)
        self._lam_dev = None                                 # on the device from the first call, like seq
        self._unfinished = None
        self.set_network(network)

    @staticmethod
    def _check_lam(x):
        x = float(x)
        if not 0.0 <= x <= 1.0:                              # (a NaN fails both comparisons)
            raise ValueError(f"lam must be in 0..1, got {x}")
        return x

    def set_network(self, network):
        """Replace the network evaluator (new weights). Launches captured with the old one
        still hold its buffers: the owner of such graphs drops them (SelfPlay.set_evaluator)."""
        if not getattr(network, "indexed", False):
            raise ValueError("MixedEvaluator: the network must evaluate a leaf list (a fused LeafEvaluator)")
        self.network = network

    @property
    def lam(self):
        return self._lam

    @lam.setter
    def lam(self, x):
        self._lam = self._check_lam(x)
        if self._lam_dev is not None:
            self._lam_dev.fill_(self._lam)

    @property
    def unfinished(self):
        """Playouts cut off by max_steps so far (0 with the default; one small device read)."""
        return 0 if self._unfinished is None else int(self._unfinished.item())

    def __call__(self, leaf_state, leaf_mask, leaf_valid, index=None, count=None):
        if self.seq is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("MixedEvaluator: the first call allocates the call counter and lambda and "
                                   "cannot be captured; call once eagerly first (SelfPlay.step does)")
            dev = self.e.device
            self.seq = torch.zeros(1, dtype=torch.int32, device=dev)
            self._lam_dev = torch.full((1,), self._lam, dtype=torch.float32, device=dev)
            self._unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
        listed = index is not None
        pi, v = self.network(leaf_state, leaf_mask, leaf_valid, index=index, count=count)
        own = None if self.rules is None else self.e.rules
        if own is not None:
            self.e.set_rules(flags=self.rules)
        try:
            self.e.playout_mix(leaf_state, self.seq, self._lam_dev, v, active=None if listed else leaf_valid,
                               index=index, count=count, policy=self.policy, playouts=self.playouts,
                               seed=self.seed, board_base=self.board_base, unfinished=self._unfinished)
        finally:
            if own is not None:
                self.e.set_rules(flags=own)
        self.seq += 1                                        # (int32 wraps as the kernel's u32 does)
        return pi, v
