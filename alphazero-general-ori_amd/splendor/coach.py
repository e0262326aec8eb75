"""Coach plug-in: Coach.executeEpisode (Coach.py:50-100) for many games at once.

`Coach(game, nnet, args, batch=B).executeEpisodes(k)` plays self-play games on B device
trees concurrently (splendor.selfplay.SelfPlay) until k games have finished, expands every
recorded position with getSymmetries (Coach.py:77-80, device kernel spl_symmetries) and
returns the reference's example records (board, pi, winner, scdiff, valids, surprise)
(Coach.py:91-98). `executeEpisode()` is the one-game form. `executeIteration(k)` returns
the same examples as a columnar `ExampleSet` and appends it to `trainExamplesHistory`
(an `ExampleHistory`, saved as .npz by `saveTrainExamples`, Coach.py:167-190); with
`args.lazy_symmetries` it keeps the positions unexpanded (`LazySymmetryExamples`) and the
variants are produced when training batches are assembled. `learn()`
is Coach.learn (Coach.py:102-164): self-play iterations, training on the example history,
the new-vs-previous BatchedArena gate and checkpoints. `args.selfplay_reserve = False` makes
the self-play games reserve-free while the gate plays the full game. `args.bootstrap_iters = k`
plays the self-play of learn()'s first k iterations with the network-free rollout search
(splendor.playout.PlayoutEvaluator on the same trees: uniform priors, leaf values from
`args.bootstrap_playouts` random playouts under `args.bootstrap_policy`), the usual cold start
from a random-init network; `use_rollout_selfplay()` is the same switch for callers that drive
executeIteration themselves and `refresh_network()` the way back. `args.rollout_mix` (a float,
or one lambda per learn() iteration) plays the iterations after the bootstrap with the mixed
evaluator (splendor.playout.MixedEvaluator: the network's priors, leaf values (1 - lambda)
v_network + lambda v_playout); `use_mixed_selfplay(lam)` is that switch.
"""
import numpy as np
import torch

from . import _lib
from .env import unpack_mask
from .arena import BatchedArena, accept_new_network
from .examples import ExampleHistory, ExampleSet, LazySymmetryExamples
from .playout import MixedEvaluator, PlayoutEvaluator
from .search import evaluator_for, nn_precision_arg
from .selfplay import SelfPlay, gather_examples


def _arg(args, k, default=None):
    if isinstance(args, dict):
        return args.get(k, default)
    return getattr(args, k, default)


def expand_symmetries(engine, ex):
    """Apply Board.get_symmetries to drained examples (device tensors, reference order);
    winner / scdiff / surprise are shared by all variants of a position."""
    if ex["board"].shape[0] == 0:
        return ex
    s, p, v, present = engine.symmetries(ex["board"], ex["pi"], ex["valids"])
    keep = present.bool()
    idx = torch.arange(ex["board"].shape[0], device=keep.device).unsqueeze(1).expand_as(keep)[keep]
    out = {"board": s[keep], "pi": p[keep], "valids": v[keep]}
    for k in ("winner", "scdiff", "surprise"):
        out[k] = ex[k][idx]
    return out


class Coach:
    def __init__(self, game, nnet, args, batch=None, seed=0x5EED, board_base=0, mem_budget=None):
        """mem_budget: bytes of HBM the self-play search arena may plan (default: most of
        what is free, BatchedMCTS._plan); learn() gives its arena gate the same bound.
        args.selfplay_reserve (default True): False plays self-play without the reserve moves
        12..26 (SplendorGame.disableReserve for the self-play handle only, the reference's
        training recipe, SplendorLogicNumba.py:96); the recorded valids and pi are the
        reserve-free tree's. The engine's rules are the same before and after.
        args.bootstrap_iters (default 0: nothing changes anywhere), args.bootstrap_playouts
        (default 4) and args.bootstrap_policy (default "buy_first"): learn()'s first iterations
        play their self-play with the rollout search (use_rollout_selfplay).
        args.rollout_mix (default 0: nothing is built): a float, or a sequence with one lambda
        per learn() iteration; an iteration after the bootstrap whose lambda is not 0 plays its
        self-play with the mixed evaluator (use_mixed_selfplay), every other one as before."""
        self.game, self.nnet, self.args = game, nnet, args
        B = int(batch or _arg(args, "numEps", 1))
        self.B = B
        self.seed, self.board_base = seed, board_base
        self.mem_budget = mem_budget
        self._rollout_ev = {}                                # (playouts, policy) -> PlayoutEvaluator
        self._mixed_ev = {}                                  # (playouts, policy) -> MixedEvaluator
        # args.selfplay_reserve = False: the self-play handle alone is reserve-free (the engine's
        # own rules are put back once it exists); the gate, the pit and check_valid play the
        # full game on the same engine: the reference's "train without, validate with"
        rules = None if _arg(args, "selfplay_reserve", True) else game.engine.rules | _lib.RULE_NO_RESERVE
        self._net_ev = evaluator_for(game.engine, nnet, B, precision=nn_precision_arg(args))
        self.sp = SelfPlay(game.engine, B, args, evaluator=self._net_ev,
                           dirichlet_noise=float(_arg(args, "dirichletAlpha", 0.0)) > 0, seed=seed,
                           board_base=board_base, mem_budget=mem_budget, rules=rules)
        self.sp.reset()
        self.trainExamplesHistory = ExampleHistory(_arg(args, "numItersHistory"))

    def run_iterations(self, k, use_graph=False):
        self.sp.run(k, use_graph=use_graph)

    def executeEpisodes(self, num_games, with_symmetries=True, as_tuples=True, gather=False):
        """Play until num_games games have finished (counted from the call), draining the
        example queue every 32 iterations. Raises EngineError if a tree froze (search path
        overflow) or finished examples were dropped. Capacity events (trees pruned under
        memory pressure) are counted in self.sp.stats()."""
        collected, done = [], 0
        start = self.sp.stats()["games_done"]
        while done < num_games:
            self.run_iterations(32)
            ex = self.sp.drain()
            if ex["board"].shape[0]:
                collected.append(ex)
            st = self.sp.stats()
            if st["overflow"]:
                raise _lib.EngineError(f"{st['overflow']} self-play trees overflowed their search path")
            done = st["games_done"] - start
        ex = {k: torch.cat([c[k] for c in collected]) for k in collected[0]} if collected else self.sp.drain()
        if gather:
            ex = gather_examples(ex)
        if with_symmetries:
            ex = expand_symmetries(self.game.engine, ex)
        if not as_tuples:
            return ex
        boards = ex["board"].cpu().numpy()
        pis = ex["pi"].cpu().numpy()
        valids = unpack_mask(ex["valids"]).cpu().numpy()
        win, sd, sur = (ex[k].cpu().numpy() for k in ("winner", "scdiff", "surprise"))
        return [(boards[i], pis[i], win[i], sd[i], valids[i], sur[i]) for i in range(len(boards))]

    def executeEpisode(self):
        return self.executeEpisodes(1)

    def executeIteration(self, num_games, with_symmetries=True, gather=False):
        """Self-play examples of one iteration (Coach.learn's executeEpisode loop,
        Coach.py:123-132) as an ExampleSet, appended to trainExamplesHistory. With
        args.lazy_symmetries the recorded positions are kept unexpanded (gathered across
        ranks as before) and a LazySymmetryExamples over them is appended instead: the same
        rows, produced when a training batch is assembled, 10-18x less memory and disk."""
        lazy = with_symmetries and bool(_arg(self.args, "lazy_symmetries", False))
        ex = self.executeEpisodes(num_games, with_symmetries=with_symmetries and not lazy, as_tuples=False,
                                  gather=gather)
        exset = ExampleSet.from_drain(ex)
        if lazy:
            exset = LazySymmetryExamples(exset, self.game.engine)
        self.trainExamplesHistory.append(exset)
        return exset

    def saveTrainExamples(self, folder=None):
        """Coach.saveTrainExamples (:167-173) without pickle: checkpoint.examples.npz."""
        return self.trainExamplesHistory.save(folder or _arg(self.args, "checkpoint", "checkpoint"))

    def loadTrainExamples(self, folder):
        """Coach.loadTrainExamples (:175-190): read checkpoint.examples.npz (either kind: a
        file of unexpanded positions comes back as lazy sets on this coach's engine)."""
        self.trainExamplesHistory = ExampleHistory.load(folder, _arg(self.args, "numItersHistory"),
                                                        device=self.game.engine.device,
                                                        engine=self.game.engine)

    def refresh_network(self):
        """Re-pack the leaf evaluator after the network's weights changed (the fused kernel
        reads a packed copy)."""
        self._net_ev = evaluator_for(self.game.engine, self.nnet, self.B, precision=nn_precision_arg(self.args))
        self.sp.set_evaluator(self._net_ev)

    def use_rollout_selfplay(self, playouts=None, policy=None):
        """Play the following self-play on the same trees with the network-free rollout search:
        the handle's evaluator becomes a PlayoutEvaluator (playouts per leaf and playout policy
        default to args.bootstrap_playouts / args.bootstrap_policy, 4 buy-first) on the Coach's
        seed and board_base and the handle's rules. The handle's simulations, cpuct, fpu, noise
        and temperature apply unchanged and the examples are recorded as always. One evaluator
        per (playouts, policy) lives as long as the Coach, so its call counter, and with it its
        Philox streams, keep advancing across iterations. refresh_network() puts the network
        evaluator back. Returns the evaluator."""
        P = int(playouts if playouts is not None else _arg(self.args, "bootstrap_playouts", 4) or 4)
        policy = policy or _arg(self.args, "bootstrap_policy", "buy_first") or "buy_first"
        ev = self._rollout_ev.get((P, policy))
        if ev is None:
            ev = self._rollout_ev[P, policy] = PlayoutEvaluator(self.game.engine, P, policy, seed=self.seed,
                                                                board_base=self.board_base, rules=self.sp.rules)
        self.sp.set_evaluator(ev)
        return ev

    def use_mixed_selfplay(self, lam, playouts=None, policy=None):
        """Play the following self-play with the mixed evaluator: the current network's priors and
        leaf values (1 - lam) v_network + lam v_playout (splendor.playout.MixedEvaluator; playouts
        per leaf and playout policy default to the bootstrap arguments, as use_rollout_selfplay,
        on the Coach's seed and board_base and the handle's rules). One evaluator per (playouts,
        policy) lives as long as the Coach and is given the latest network evaluator, so its call
        counter keeps advancing across refresh_network(). While it is the handle's evaluator on
        the current network, another lam only writes the device scalar and the captured graphs
        stay; otherwise it goes in through set_evaluator. refresh_network() puts the plain network
        evaluator back. Returns the evaluator."""
        P = int(playouts if playouts is not None else _arg(self.args, "bootstrap_playouts", 4) or 4)
        policy = policy or _arg(self.args, "bootstrap_policy", "buy_first") or "buy_first"
        ev = self._mixed_ev.get((P, policy))
        if ev is None:
            ev = self._mixed_ev[P, policy] = MixedEvaluator(self.game.engine, self._net_ev, P, policy, lam=lam,
                                                            seed=self.seed, board_base=self.board_base,
                                                            rules=self.sp.rules)
        ev.lam = lam
        if self.sp.evaluator is not ev or ev.network is not self._net_ev:
            ev.set_network(self._net_ev)
            self.sp.set_evaluator(ev)
        return ev

    def _mix_lambda(self, i):
        """args.rollout_mix for learn()'s iteration i (1-based): 0 when absent or past the end."""
        mix = _arg(self.args, "rollout_mix", 0) or 0
        if isinstance(mix, (int, float)):
            return float(mix)
        return float(mix[i - 1]) if i <= len(mix) else 0.0

    def learn(self, pnet=None, log=None):
        """Coach.learn (Coach.py:102-164): for numIters iterations, numEps self-play games
        (fresh games and trees, as the reference's executeEpisode + reset_all_search_trees),
        the example history saved, the network trained on it, then pitted against the
        previous weights over arenaCompare games (BatchedArena, temp 0, full searches) and
        kept iff it wins >= updateThreshold of the decisive games (under torch.distributed
        every rank's examples are all-gathered first, so all ranks train on the same set);
        checkpoints as
        checkpoint_<i>.pt / best.pt / temp.pt in args.checkpoint. In iterations i <=
        args.bootstrap_iters the self-play runs on the rollout search (use_rollout_selfplay);
        training, the gate and the checkpoints are the same, and the network evaluator is back
        after the iteration. A later iteration whose args.rollout_mix entry is not 0 plays on the
        mixed evaluator in the same way (use_mixed_selfplay). Returns per-iteration (nwins, pwins, draws, accepted)."""
        from .NNet import NNetWrapper
        folder = _arg(self.args, "checkpoint", "checkpoint")
        pnet = pnet or NNetWrapper(self.game, dict(self.nnet.args), device=self.nnet.device)
        history = []
        bootstrap = int(_arg(self.args, "bootstrap_iters", 0) or 0)
        for i in range(1, int(_arg(self.args, "numIters", 1)) + 1):
            if not _arg(self.args, "skipFirstSelfPlay", False) or i > 1:
                if i <= bootstrap:
                    self.use_rollout_selfplay()
                elif self._mix_lambda(i) != 0:
                    self.use_mixed_selfplay(self._mix_lambda(i))
                self.sp.reset()
                self.executeIteration(int(_arg(self.args, "numEps", self.B)), gather=True)
            self.saveTrainExamples(folder)
            self.nnet.save_checkpoint(folder=folder, filename="temp.pt")
            pnet.load_checkpoint(folder=folder, filename="temp.pt")
            self.nnet.train(self.trainExamplesHistory.merged())
            games = int(_arg(self.args, "arenaCompare", 2))
            arena = BatchedArena(self.game, self.nnet, pnet, self.args, batch=min(games, self.B),
                                 seed=self.seed + i, mem_budget=self.mem_budget)
            nwins, pwins, draws = arena.playGames(games)
            ok = accept_new_network(nwins, pwins, float(_arg(self.args, "updateThreshold", 0.55)))
            if ok:
                self.nnet.save_checkpoint(folder=folder, filename=f"checkpoint_{i}.pt")
                self.nnet.save_checkpoint(folder=folder, filename="best.pt")
            else:
                self.nnet.load_checkpoint(folder=folder, filename="temp.pt")
            self.refresh_network()
            history.append((nwins, pwins, draws, ok))
            if log:
                log(f"iter {i}: new vs previous {nwins}-{pwins} ({draws} draws) -> "
                    f"{'ACCEPTED' if ok else 'REJECTED'}")
        return history
