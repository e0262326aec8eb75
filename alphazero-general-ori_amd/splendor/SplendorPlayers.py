"""The reference's rule-based players (SplendorPlayers.py:18-25, :93-115) for the sequential
Arena and pit.py-style code: `RandomPlayer(game).play` and `GreedyPlayer(game).play` take a
canonical board and return an action. Each call is the batched players' kernel
(spl_player_move, splendor.pit) on a one-board batch, so both forms choose by one rule.

The choice among a player's candidates is the Philox draw (game.seed, board 0, stream =
the game's call counter), as SplendorGame keys its own chance draws, where the reference
calls the unseeded `random`. The human and alpha-beta players are out of scope.
"""
from . import _lib


class _RulePlayer:
    kind = None

    def __init__(self, game):
        self.game = game

    def _move(self, board):
        g = self.game
        out = g.engine.player_move(g._t(board), self.kind, seed=g.seed, stream=g._stream(), board_base=0)
        return int(out.item())


class RandomPlayer(_RulePlayer):
    """Uniform over the legal moves of `player` (:18-25)."""
    kind = _lib.PLAYER_RANDOM

    def play(self, board, player=0):
        return self._move(self.game.getCanonicalForm(board, player))


class GreedyPlayer(_RulePlayer):
    """A move that scores the most points now; when none scores, a visible buy, else a
    take-gems move, else any legal move (:93-115; the lookahead scores the mover and is
    deterministic)."""
    kind = _lib.PLAYER_GREEDY

    def play(self, board):
        return self._move(board)


__all__ = ["RandomPlayer", "GreedyPlayer"]
