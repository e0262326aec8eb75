#!/usr/bin/env python3
"""review.py / analyze.py on the batched engine: search every position of recorded games with
a large budget and report, per turn, the value, the policy entropy, the played move against the
search's choice and the principal variation.

    python3 tools/pit.py -p checkpoint/best.pt greedy -n 64 -m 100 --record out/games.npz
    python3 tools/review.py out/games.npz -p checkpoint/best.pt -m 1600 -c 2.5 -f 0.3 --csv out/review.csv
    python3 tools/review.py out/games.npz -p rollout:buy_first:4 -m 400 --games 0:8 --lines 3 --depth 8

RECORD.npz is what tools/pit.py --record writes (BatchedPit.record()). The reviewer (-p) is any
player spec of tools/pit.py that searches: a checkpoint, `init`, `rollout:...` or `mixed:...`,
with -m simulations per position (analyze.py uses 10,000) and -c / -f as cpuct / fpu. All
positions of the chosen games (--games A:B, record rows A..B-1; default all) are independent
roots of one batched search (--batch trees at a time); the lines below the root are read from
the stored trees (BatchedMCTS.principal_variations), nothing is re-rooted. The games are
replayed from the record's seed first, and the replay must reproduce their results and scores.

--csv writes one row per position: game, ply, round, mover, the per-seat scores, value (the
root value for the mover), entropy of the visit distribution, the played move with its visits,
visit share, rank and Q, the search's best move with its visits, share and Q, q_loss = Q(best)
- Q(played) (empty when the played move was not visited), and line 0 as a move string. Stdout
lists the --top positions with the largest q_loss of every game. The board display, the record
directory format of the reference's pit.py and the plots of analyze.py are out of scope."""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("record", metavar="RECORD.npz")
    ap.add_argument("--player", "-p", required=True, metavar="player", help="the reviewer (a tools/pit.py spec)")
    ap.add_argument("--numMCTSSims", "-m", type=int, required=True)
    ap.add_argument("--cpuct", "-c", type=float, default=None)
    ap.add_argument("--fpu", "-f", type=float, default=None)
    ap.add_argument("--games", default=None, metavar="A:B", help="record rows A..B-1 (default: all)")
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--batch", type=int, default=None, help="positions searched at once (default: all, at most 4096)")
    ap.add_argument("--top", type=int, default=3, help="positions listed per game")
    ap.add_argument("--csv", default=None, metavar="OUT.csv")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    from pit import create_player
    from splendor import _lib
    from splendor.SplendorGame import SplendorGame, move_to_str
    from splendor.arena import arena_mcts_args
    from splendor.review import evaluator_of, line_string, review
    with np.load(a.record) as z:
        rec = {k: z[k] for k in z.files}
    game = SplendorGame(int(rec["n"]))
    game.engine.set_token_limit(int(rec["token_limit"]))
    game.engine.set_rules(flags=int(rec["rules"]))
    G = len(rec["game"])
    rows = np.arange(G)
    if a.games:
        lo, _, hi = a.games.partition(":")
        rows = rows[int(lo or 0):int(hi) if hi else G]
    n_pos = int(np.asarray(rec["plies"])[rows].sum())
    batch = int(a.batch or min(max(n_pos, 1), 4096))
    spec = create_player(a.player, game, a.numMCTSSims, a.cpuct, a.fpu)
    margs = arena_mcts_args(None, numMCTSSims=a.numMCTSSims, cpuct=a.cpuct, fpu=a.fpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = review(game, evaluator_of(game.engine, spec, batch), rec, margs, games=rows, lines=a.lines, depth=a.depth,
                 batch=batch)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    N, n = len(out["ply"]), game.engine.n
    line0 = [line_string(out["pv_action"][i, 0], out["pv_length"][i, 0]) for i in range(N)]

    def num(x):
        return "" if np.isnan(x) else f"{x:.6g}"
    if a.csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.csv)), exist_ok=True)
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["game", "ply", "round", "mover"] + [f"score{p}" for p in range(n)] +
                       ["value", "entropy", "played", "played_move", "played_visits", "played_share", "played_rank",
                        "played_q", "best", "best_move", "best_visits", "best_share", "best_q", "q_loss", "line0"])
            for i in range(N):
                w.writerow([int(out["game"][i]), int(out["ply"][i]), int(out["ply"][i]) // n, int(out["mover"][i])] +
                           [int(s) for s in out["scores"][i]] +
                           [num(out["value"][i]), num(out["entropy"][i]), int(out["played"][i]),
                            move_to_str(int(out["played"][i])), int(out["played_visits"][i]),
                            num(out["played_share"][i]), int(out["played_rank"][i]), num(out["played_q"][i]),
                            int(out["best"][i]), move_to_str(int(out["best"][i])), int(out["best_visits"][i]),
                            num(out["best_share"][i]), num(out["best_q"][i]), num(out["q_loss"][i]), line0[i]])
    print(f"{a.player} reviews {len(rows)} games, {N} positions, {a.numMCTSSims} simulations each: "
          f"{seconds:.1f} s ({N / max(seconds, 1e-9):.0f} positions/s)")
    ends = np.bincount(out["pv_end"][:, 0], minlength=_lib.PV_END_NONE + 1) if N else np.zeros(5, int)
    print("line 0 ends: " + ", ".join(f"{k} {int(v)}" for k, v in zip(("depth", "unlinked", "terminal", "unvisited",
                                                                       "none"), ends)))
    for r in rows:
        g = int(rec["game"][r])
        sel = np.flatnonzero(out["row"] == r)
        loss = np.where(np.isnan(out["q_loss"][sel]), -np.inf, out["q_loss"][sel])
        mean = float(loss[np.isfinite(loss)].mean()) if np.isfinite(loss).any() else float("nan")
        print(f"game {g}: {int(rec['plies'][r])} plies, result {rec['result'][r].tolist()}, "
              f"score {rec['score'][r].tolist()}, mean q_loss {mean:.3f}")
        for j in np.argsort(-loss, kind="stable")[:a.top]:
            i = sel[j]
            if not np.isfinite(loss[j]):
                break
            print(f"  ply {int(out['ply'][i]):3d} seat {int(out['mover'][i])} value {out['value'][i]:+.3f}  played "
                  f"{move_to_str(int(out['played'][i]))} ({out['played_share'][i]:.0%}, rank {int(out['played_rank'][i])})"
                  f"  q_loss {out['q_loss'][i]:.3f}  best: {line0[i]}")
    return out


if __name__ == "__main__":
    main()
