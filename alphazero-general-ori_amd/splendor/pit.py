"""Batched pit (pit.py:32-96 with the players of SplendorPlayers.py): any two of a search
player, a raw-policy player, the greedy player and the random player, over many games at
once on the device.

    BatchedPit(game, MCTSPlayer(nnet, numMCTSSims=100), GreedyPlayer(), batch=4096).playGames(4096)
    -> (oneWon, twoWon, draws); per-game records in `.last`

Player specs (what pit.py's create_player builds from a name):
* MCTSPlayer(nnet, numMCTSSims=, cpuct=, fpu=, nn_precision=, evaluator=None): a search
  player with its own BatchedMCTS and its own search arguments (pit.py:74-82, ai_1 / ai_2
  with different numMCTSSims); arguments left None come from the pit's `args`;
* RolloutPlayer(numMCTSSims=, playouts=1, policy="buy_first", cpuct=, fpu=): a search player
  that needs no network: the same search with uniform priors and leaf values from random
  playouts (splendor.playout.PlayoutEvaluator, one spl_playout launch per simulation). Its
  strength is set by simulations per move and playouts per leaf: a fixed yardstick between
  the random and the greedy player and beyond;
* MixedPlayer(nnet, lam, playouts=1, policy="buy_first", numMCTSSims=, cpuct=, fpu=,
  nn_precision=): a search player seated like MCTSPlayer whose leaves get the network's priors
  and the value (1 - lam) v_network + lam v_playout (splendor.playout.MixedEvaluator); at lam =
  0 it moves exactly as MCTSPlayer(nnet);
* PolicyPlayer(nnet, evaluator=None): the arg-max of the network's policy over the legal
  moves, no search;
* GreedyPlayer(): SplendorPlayers.py:93-115, scoring the mover;
* RandomPlayer(): SplendorPlayers.py:18-25.
The last three move by one spl_player_move launch per ply and allocate no tree.
A RolloutPlayer (and a MixedPlayer) draws its playouts with its search seed (seed ^ (k + 1)), board = game_base +
slot * playouts + playout, streams 256 c .. for its c-th simulation: a run repeats exactly.

Every player follows the engine's rules as they are when the pit is created (after
game.disableReserve() nobody plays 12..26); they must not change while the pit lives (splendor.arena).
The ply loop, the game order 1 2 2 1, the seats for n > 2, the deals and chance streams, the
check_valid assertion and the capacity warning are BatchedArena's (splendor.arena): the pit
only seats other player objects. Player k (0, 1) draws with seed ^ (k + 1), board =
game_base + global game id, stream = ply: a search player's tie-break exactly as in
BatchedArena, the other players' choice among their candidates.
"""
import torch

from . import _lib
from .arena import BatchedArena, TreePlayer, _arg, arena_mcts_args
from .mcts import BatchedMCTS
from .playout import MixedEvaluator, PlayoutEvaluator
from .search import evaluator_for, nn_precision_arg


class MCTSPlayer:
    def __init__(self, nnet, numMCTSSims=None, cpuct=None, fpu=None, nn_precision=None, evaluator=None):
        self.nnet, self.evaluator, self.nn_precision = nnet, evaluator, nn_precision
        self.own = dict(numMCTSSims=numMCTSSims, cpuct=cpuct, fpu=fpu)


class RolloutPlayer:
    def __init__(self, numMCTSSims=None, playouts=1, policy="buy_first", cpuct=None, fpu=None):
        self.playouts, self.policy = int(playouts), policy
        self.own = dict(numMCTSSims=numMCTSSims, cpuct=cpuct, fpu=fpu)


class MixedPlayer:
    evaluator = None

    def __init__(self, nnet, lam, playouts=1, policy="buy_first", numMCTSSims=None, cpuct=None, fpu=None,
                 nn_precision=None):
        self.nnet, self.lam, self.nn_precision = nnet, MixedEvaluator._check_lam(lam), nn_precision
        self.playouts, self.policy = int(playouts), policy
        self.own = dict(numMCTSSims=numMCTSSims, cpuct=cpuct, fpu=fpu)


class PolicyPlayer:
    def __init__(self, nnet, evaluator=None):
        self.nnet, self.evaluator = nnet, evaluator


class GreedyPlayer:
    kind = _lib.PLAYER_GREEDY


class RandomPlayer:
    kind = _lib.PLAYER_RANDOM


class RulePlayer:
    """A seated greedy / random player: one spl_player_move launch per ply."""

    def __init__(self, engine, kind, seed):
        self.e, self.kind, self.seed = engine, kind, seed

    def new_games(self, boards):
        pass

    def move(self, canon, active, base, ply, out):
        self.e.player_move(canon, self.kind, active=active, seed=self.seed, stream=ply, board_base=base, out=out)


class PriorPlayer:
    """A seated raw-policy player: the network on every board of the batch (as a search
    evaluates its leaves), then the arg-max over the legal moves, ties by the keyed draw."""

    def __init__(self, engine, evaluator, seed):
        self.e, self.evaluator, self.seed = engine, evaluator, seed

    def new_games(self, boards):
        pass

    def move(self, canon, active, base, ply, out):
        pi, _ = self.evaluator(canon, self.e.valid_moves(canon), active)
        self.e.player_move(canon, _lib.PLAYER_POLICY, active=active, pi=pi.float().contiguous(), seed=self.seed,
                           stream=ply, board_base=base, out=out)


class BatchedPit(BatchedArena):
    def __init__(self, game, player1, player2, args=None, batch=None, seed=0x5EED, game_base=0,
                 check_valid=True, mem_budget=None):
        self.game, self.args = game, args
        self.e = game.engine
        self.n = self.e.n
        self.B = int(batch or _arg(args, "arenaCompare", 1))
        self.seed, self.game_base = int(seed), int(game_base)
        self.check_valid = check_valid
        specs = (player1, player2)
        # the networks first, then the trees share the memory that is left (as BatchedArena)
        evs = [self._evaluator(s) for s in specs]
        trees = sum(isinstance(s, (MCTSPlayer, RolloutPlayer, MixedPlayer)) for s in specs)
        budget = None
        if trees and mem_budget:
            budget = int(mem_budget) // trees
        elif trees and self.e.device.type == "cuda":
            budget = int(0.8 / trees * torch.cuda.mem_get_info(self.e.device)[0])
        self.players = [self._seat(k, s, evs[k], budget) for k, s in enumerate(specs)]
        self.mcts = [p.mcts for p in self.players if isinstance(p, TreePlayer)]
        self.last = None
        self.capacity = {"prunes": 0, "resets": 0, "unexpanded": 0}

    def _evaluator(self, spec):
        if not isinstance(spec, (MCTSPlayer, MixedPlayer, PolicyPlayer)):
            return None
        if spec.evaluator is not None:
            return spec.evaluator
        prec = getattr(spec, "nn_precision", None) or nn_precision_arg(self.args)
        if not isinstance(prec, str):
            raise ValueError("nn_precision: a pit player takes one mode (give each MCTSPlayer its own)")
        return evaluator_for(self.e, spec.nnet, self.B, precision=prec)

    def _seat(self, k, spec, evaluator, budget):
        seed = self.mcts_seed(k)
        if isinstance(spec, MixedPlayer):
            evaluator = MixedEvaluator(self.e, evaluator, spec.playouts, spec.policy, lam=spec.lam, seed=seed,
                                       board_base=self.game_base)
        if isinstance(spec, (MCTSPlayer, MixedPlayer)):
            return TreePlayer(BatchedMCTS(self.e, self.B, arena_mcts_args(self.args, **spec.own), evaluator,
                                          dirichlet_noise=False, seed=seed, board_base=self.game_base,
                                          mem_budget=budget))
        if isinstance(spec, RolloutPlayer):
            ev = PlayoutEvaluator(self.e, spec.playouts, spec.policy, seed=seed, board_base=self.game_base)
            return TreePlayer(BatchedMCTS(self.e, self.B, arena_mcts_args(self.args, **spec.own), ev,
                                          dirichlet_noise=False, seed=seed, board_base=self.game_base,
                                          mem_budget=budget))
        if isinstance(spec, PolicyPlayer):
            return PriorPlayer(self.e, evaluator, seed)
        if isinstance(spec, (GreedyPlayer, RandomPlayer)):
            return RulePlayer(self.e, spec.kind, seed)
        raise TypeError(f"player {k + 1}: expected MCTSPlayer, RolloutPlayer, MixedPlayer, PolicyPlayer, "
                        f"GreedyPlayer or RandomPlayer, got {type(spec).__name__}")
