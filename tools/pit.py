#!/usr/bin/env python3
"""pit.py (pit.py:32-96, :225-246) on the batched engine: play two agents against each other
over many games at once and print (oneWon, twoWon, draws).

    python3 tools/pit.py --players greedy random -n 4096
    python3 tools/pit.py -p checkpoint/best.pt greedy -n 4096 -m 100 -c 2.5 -f 0.3 --json out.json
    python3 tools/pit.py -p a.pt a.pt -m1 50 -m2 200              # pit.py's ai_1 / ai_2
    python3 tools/pit.py -p rollout:buy_first:4 greedy -n 1024 -m 100 -c 2.5 -f 0.3
    python3 tools/pit.py -p mixed:checkpoint/best.pt:0.5:buy_first:4 greedy -n 1024 -m 100 -c 2.5 -f 0.3

A player is `random`, `greedy` (SplendorPlayers.py), a checkpoint path (search with -m / -c /
-f, as pit.py's create_player), `policy:<checkpoint>` (the network's arg-max policy, no
search), `init` / `policy:init` (the seeded random-init network, a floor for trained
ones), or `rollout` / `rollout:<policy>:<playouts>` (the search without a network: uniform
priors, leaf values from <playouts> random playouts, policy uniform or buy_first; default
buy_first:1; simulations from -m / -m1 / -m2), or `mixed:<checkpoint>:<lambda>` /
`mixed:<checkpoint>:<lambda>:<policy>:<playouts>` (the checkpoint's search with leaf values (1 -
lambda) v_network + lambda v_playout; default buy_first:1). Checkpoints load through NNetWrapper.load_checkpoint (weights only). Every game is
played on the device (splendor.pit.BatchedPit): --batch games at a time, Philox-keyed by
--seed, so a run repeats exactly. --no-reserve plays the reserve-free game (actions 12..26
never legal, the reference's training-time rule) for both players. --json appends the run's record (players, settings,
wins / losses / draws, mean plies, wall seconds) to the JSON list in that file. --record FILE.npz saves every game
move for move (BatchedPit.record() plus the player specs and search arguments) for tools/review.py. The human and
alpha-beta players, ratings and the board display of pit.py are out of scope."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-general-ori_amd"))


def create_player(name, game, sims, cpuct, fpu):
    """pit.py:32-94 create_player: a BatchedPit player spec from a name."""
    from splendor import pit
    from splendor.NNet import NNetWrapper
    if name == "random":
        return pit.RandomPlayer()
    if name == "greedy":
        return pit.GreedyPlayer()
    if name == "rollout" or name.startswith("rollout:"):
        part = name.split(":")
        if len(part) not in (1, 3):
            raise SystemExit(f"{name}: expected rollout or rollout:<policy>:<playouts>")
        kw = dict(policy=part[1], playouts=int(part[2])) if len(part) == 3 else {}
        return pit.RolloutPlayer(numMCTSSims=sims, cpuct=cpuct, fpu=fpu, **kw)
    policy, mixed = name.startswith("policy:"), name.startswith("mixed:")
    path = name[len("policy:"):] if policy else name
    if mixed:
        part = name.split(":")
        if len(part) not in (3, 5):
            raise SystemExit(f"{name}: expected mixed:<checkpoint>:<lambda>[:<policy>:<playouts>]")
        path, lam = part[1], float(part[2])
        kw = dict(policy=part[3], playouts=int(part[4])) if len(part) == 5 else {}
    if os.path.isdir(path):
        path = os.path.join(path, "best.pt")                 # pit.py:97
    net = NNetWrapper(game, dict(dropout=0.0), seed=0)
    if path != "init":
        net.load_checkpoint(*os.path.split(path))
    if policy:
        return pit.PolicyPlayer(net)
    if mixed:
        return pit.MixedPlayer(net, lam, numMCTSSims=sims, cpuct=cpuct, fpu=fpu, **kw)
    return pit.MCTSPlayer(net, numMCTSSims=sims, cpuct=cpuct, fpu=fpu)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--players", "-p", nargs=2, required=True, metavar="player")
    ap.add_argument("--num-games", "-n", type=int, default=30)
    ap.add_argument("--numMCTSSims", "-m", type=int, default=None)
    ap.add_argument("--numMCTSSims1", "-m1", type=int, default=None, help="player 1's simulations")
    ap.add_argument("--numMCTSSims2", "-m2", type=int, default=None, help="player 2's simulations")
    ap.add_argument("--cpuct", "-c", type=float, default=None)
    ap.add_argument("--fpu", "-f", type=float, default=None)
    ap.add_argument("--num-players", "-N", type=int, default=2, choices=(2, 3, 4),
                    help="seats of the game (seat 0 one player, every other seat the other)")
    ap.add_argument("--batch", type=int, default=None, help="games played at once (default: all)")
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--no-reserve", action="store_true",
                    help="play without the reserve moves 12..26 (SplendorGame.disableReserve)")
    ap.add_argument("--json", default=None, metavar="FILE", help="append the run's record to this JSON list")
    ap.add_argument("--record", default=None, metavar="FILE.npz",
                    help="save the games (every move, with the deal and chance keys) for tools/review.py")
    a = ap.parse_args(argv)

    import torch
    from splendor.SplendorGame import SplendorGame
    from splendor.pit import BatchedPit
    game = SplendorGame(a.num_players)
    if a.no_reserve:
        game.disableReserve()
    sims = [s if s is not None else a.numMCTSSims for s in (a.numMCTSSims1, a.numMCTSSims2)]
    players = [create_player(p, game, sims[k], a.cpuct, a.fpu) for k, p in enumerate(a.players)]
    batch = min(a.batch or a.num_games, a.num_games)
    pit = BatchedPit(game, players[0], players[1], None, batch=batch, seed=a.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one, two, draws = pit.playGames(a.num_games)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(a.players[0], "vs", a.players[1])
    print((one, two, draws))
    rec = {"players": list(a.players), "num_players": a.num_players, "games": a.num_games, "batch": batch,
           "seed": a.seed, "no_reserve": a.no_reserve, "numMCTSSims": sims, "cpuct": a.cpuct, "fpu": a.fpu, "one_won": one, "two_won": two,
           "draws": draws, "mean_plies": float(pit.last["plies"].mean()), "seconds": seconds,
           "capacity_events": pit.capacity}
    print(json.dumps(rec), flush=True)
    if a.record:
        # BatchedPit.record() (what splendor.review.replay needs) + who played and how they searched
        import numpy as np
        os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
        none = float("nan")
        np.savez_compressed(a.record, **pit.record(), players=np.array(a.players),
                            numMCTSSims=np.array([-1 if s is None else s for s in sims], dtype=np.int64),
                            cpuct=np.float64(none if a.cpuct is None else a.cpuct),
                            fpu=np.float64(none if a.fpu is None else a.fpu))
    if a.json:
        runs = []
        if os.path.exists(a.json):
            with open(a.json) as f:
                runs = json.load(f)
        runs.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)
            f.write("\n")
    return rec


if __name__ == "__main__":
    main()
