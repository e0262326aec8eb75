#!/usr/bin/env python3
"""Golden positions for the rule-based players (runs ONLY in the build container, like
make_golden.py, whose loaders it imports: the reference's Board is executed in memory and
only the arrays below are written).

tests/golden/players_{2,3,4}p.npz, at most 256 canonical positions each (the mover is
player 0), taken from seeded random-play games:
    board  int8  [P,R,7]
    valid  uint8 [P,409]   the reference's valid_moves(0)
    s0     int16 [P]       the reference's get_score(0)
    after  int16 [P,409]   get_score(0) after make_move(a, 0, True) on a copy for every
                           legal a, -1 elsewhere
    cls    uint8 [P]       bit k set: the position is in class k of CLASSES
Classes (what the greedy player's rule branches on, SplendorPlayers.py:105-113, with the
mover scored), m = max of `after` over the legal moves:
    0  m > s0 and at least two scoring moves of different gain
    1  m > s0 and a tie for the maximum
    2  no scoring move, a visible buy (0-11) is legal
    3  no scoring move, no visible buy, a take-gems move (30-59) is legal
    4  no scoring move, no visible buy, no take-gems move
Random play does not reach class 4: those positions are class-3 positions whose bank
colour counts are zeroed before the reference sees them. The generator fails unless every
class has at least MIN_PER_CLASS positions.

Usage:  python tests/golden/make_players_golden.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402

CLASSES = 5
MIN_PER_CLASS = 8
QUOTA = (48, 48, 64, 64, 16)          # positions kept per class (a position may count for two)
MAX_POSITIONS = 256
MAX_GAMES = 300


def classify(valid, s0, after):
    legal = np.flatnonzero(valid)
    s = after[legal]
    m = int(s.max())
    if m > s0:
        scoring = s[s > s0]
        return (1 if len(np.unique(scoring)) >= 2 else 0) | (2 if int((s == m).sum()) >= 2 else 0)
    if valid[:12].any():
        return 4
    return 8 if valid[30:60].any() else 16


def describe(Board, n, board):
    """(valid, s0, after) of a canonical position, from the reference."""
    b = Board(n)
    b.copy_state(board, True)
    valid = b.valid_moves(0).astype(np.uint8)
    b.copy_state(board, True)
    s0 = int(b.get_score(0))
    after = np.full(409, -1, np.int16)
    for a in np.flatnonzero(valid):
        b.copy_state(board, True)
        b.make_move(int(a), 0, True)
        after[a] = int(b.get_score(0))
    return valid, s0, after


def positions(numba_logic, n, seed):
    Board = numba_logic.Board
    rng = np.random.default_rng(seed)
    rec = {k: [] for k in ("board", "valid", "s0", "after", "cls")}
    count = [0] * CLASSES

    def keep(board, valid, s0, after, c):
        for k, v in zip(("board", "valid", "s0", "after", "cls"), (board.copy(), valid, s0, after, c)):
            rec[k].append(v)
        for k in range(CLASSES):
            count[k] += (c >> k) & 1

    def wanted(c):
        return any((c >> k) & 1 and count[k] < QUOTA[k] for k in range(CLASSES))

    room = MAX_POSITIONS - QUOTA[4]
    for g in range(MAX_GAMES):
        if all(count[k] >= QUOTA[k] for k in range(4)) or len(rec["board"]) >= room:
            break
        MG.STREAM.set_source(np.random.default_rng([seed, g, 1]))
        b = Board(n)
        state, player = b.get_state().copy(), 0
        scratch = Board(n)
        for ply in range(62 * n + 8):
            scratch.copy_state(state, True)
            if player:
                scratch.swap_players(player)
            canon = scratch.get_state().copy()
            valid, s0, after = describe(Board, n, canon)
            c = classify(valid, s0, after)
            if wanted(c) and len(rec["board"]) < room:
                keep(canon, valid, s0, after, c)
            legal = np.flatnonzero(valid)
            a = int(legal[rng.integers(len(legal))])
            MG.STREAM.set_source(np.random.default_rng([seed, g, 2, ply]))
            scratch.copy_state(state, True)
            player = scratch.make_move(a, player, False)
            state = scratch.get_state().copy()
            if scratch.check_end_game().any():
                break
    # class 4: the bank's colour counts of class-3 positions zeroed
    for i in [i for i, c in enumerate(rec["cls"]) if c == 8]:
        if count[4] >= QUOTA[4]:
            break
        board = rec["board"][i].copy()
        board[0, :5] = 0
        valid, s0, after = describe(Board, n, board)
        c = classify(valid, s0, after)
        if c == 16:
            keep(board, valid, s0, after, c)
    if min(count) < MIN_PER_CLASS:
        raise SystemExit(f"{n}p: class counts {count}: fewer than {MIN_PER_CLASS} positions in a class")
    out = {"board": np.array(rec["board"], np.int8), "valid": np.array(rec["valid"], np.uint8),
           "s0": np.array(rec["s0"], np.int16), "after": np.array(rec["after"], np.int16),
           "cls": np.array(rec["cls"], np.uint8)}
    return out, count


def main():
    _, numba_logic, _, _ = MG.load_reference()
    MG._patch_np_random()
    for n in (2, 3, 4):
        out, count = positions(numba_logic, n, seed=7100 + n)
        path = os.path.join(OUT, f"players_{n}p.npz")
        np.savez_compressed(path, **out)
        print(f"players {n}p: {len(out['board'])} positions, class counts {count}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
