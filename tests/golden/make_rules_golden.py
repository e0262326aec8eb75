#!/usr/bin/env python3
"""Golden vectors of the reserve-free game (runs ONLY in the build container, like
make_golden.py, whose loaders and fixture functions it imports unchanged: the reference is
executed in memory and only the arrays below are written).

The reference's switch is Board.ENABLE_ACTION_RESERVE (SplendorLogicNumba.py:96, read by
_valid_reserve(is_limit=True), :508-510; SplendorGame.disableReserve, SplendorGame.py:82-83).
Here a Board subclass sets it to False in its constructor and a SplendorGame subclass calls
disableReserve(); make_golden's fixture functions receive them through SimpleNamespace shims
in place of the modules they take, so every recorded mask, search and episode is the
reference's under the switch:

    noreserve_env_{2,3,4}p.npz      env_fixtures, 6 random reserve-free games: state, player,
                                    canon, mask_canon, mask_player, action, next_state,
                                    next_player, u_off, u_len, uniforms
    noreserve_mcts_{2,4}p.npz       mcts_fixtures, cases (25, 1.0, 0.0, plain), (100, 2.5, 0.3,
                                    plain), (100, 2.5, 0.3, forced): 18 searches and a 30-move
                                    game with tree reuse
    noreserve_episode_{2p,4p}.npz   episode_fixtures with make_golden's episode arguments,
                                    boards (3,) at 2 players and (2,) at 4

The generator fails unless the fixtures cover what the rule changes and what it must leave
alone: no mask bit, root visit or played action in 12..26 anywhere; reserve + give (290..364)
legal in some env position of every player count, visited by the searches and played in the
4-player episode; a pass (408) in some 3- or 4-player env position.

Usage:  python tests/golden/make_rules_golden.py
"""
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402

ENV_KEYS = ("state", "player", "canon", "mask_canon", "mask_player", "action", "next_state", "next_player",
            "u_off", "u_len", "uniforms")
ENV_MAX_BYTES = 168 * 1024          # env_2p.npz's size
MCTS_CASES = [(25, 1.0, 0.0, False), (100, 2.5, 0.3, False), (100, 2.5, 0.3, True)]
# make_golden.main's episode arguments
EARGS = {"numMCTSSims": 24, "cpuct": 1.5, "fpu": 0.1, "prob_fullMCTS": 0.5, "ratio_fullMCTS": 4,
         "forced_playouts": False, "no_mem_optim": False, "dirichletAlpha": 0.3,
         "temperature": [1.25, 0.8], "tempThreshold": 10, "no_compression": True}
RSV = slice(12, 27)
RSV_GIVE = slice(290, 365)
PASS = 408


def no_reserve_shims(numba_logic, game_mod):
    class Board(numba_logic.Board):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.ENABLE_ACTION_RESERVE = False

    class SplendorGame(game_mod.SplendorGame):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.disableReserve()

    return types.SimpleNamespace(Board=Board), types.SimpleNamespace(SplendorGame=SplendorGame)


def save(name, arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path)


def main():
    _, numba_logic, game_mod, mcts_mod = MG.load_reference()
    MG._patch_np_random()
    logic_shim, game_shim = no_reserve_shims(numba_logic, game_mod)
    passes = 0
    for n in (2, 3, 4):
        env = MG.env_fixtures(logic_shim, n, 6, seed=8000 + n)
        total = len(env["state"])
        masks = np.concatenate([env["mask_canon"], env["mask_player"]])
        assert not masks[:, RSV].any(), f"{n}p: a reserve bit under the switch"
        give = int(env["mask_canon"][:, RSV_GIVE].any(1).sum())
        assert give, f"{n}p: reserve + give never legal"
        npass = int(env["mask_canon"][:, PASS].sum())
        passes += npass if n > 2 else 0
        size = save(f"noreserve_env_{n}p.npz", {k: env[k] for k in ENV_KEYS})
        assert size <= ENV_MAX_BYTES, f"{n}p: {size} bytes: subsample the positions"
        print(f"noreserve env {n}p: {total} positions, reserve + give legal in {give}, "
              f"pass in {npass}, {size} bytes")
    assert passes, "no pass position at 3 or 4 players"
    for n in (2, 4):
        mf = MG.mcts_fixtures(game_shim, mcts_mod, logic_shim, n, seed=8100 + n, cases=MCTS_CASES)
        counts = np.concatenate([mf["counts"], mf["seq_counts"]])
        assert not counts[:, RSV].any(), f"{n}p: root visits on reserve moves"
        give = int(counts[:, RSV_GIVE].sum())
        assert give, f"{n}p: no root visit on reserve + give"
        assert not np.isin(mf["seq_action"], np.arange(12, 27)).any()
        size = save(f"noreserve_mcts_{n}p.npz", mf)
        print(f"noreserve mcts {n}p: {len(mf['root'])} searches, seq moves {len(mf['seq_root'])}, "
              f"visits on reserve + give {give}, {size} bytes")
    coach_mod = MG.load_coach()
    for n, boards in ((2, (3,)), (4, (2,))):
        ef = MG.episode_fixtures(game_shim, coach_mod, n, 0x5EED + n, boards, dict(EARGS))
        acts = ef["game_actions"][ef["game_actions"] >= 0]
        assert not ef["valids"][:, RSV].any() and not ef["pi"][:, RSV].any(), f"{n}p: reserve in an example"
        assert not np.isin(acts, np.arange(12, 27)).any(), f"{n}p: a reserve move was played"
        give, npass = int(np.isin(acts, np.arange(290, 365)).sum()), int((acts == PASS).sum())
        if n == 4:
            assert give, "4p episode: no reserve + give move"
        size = save(f"noreserve_episode_{n}p.npz", ef)
        print(f"noreserve episode {n}p: moves {ef['game_moves'].tolist()}, examples "
              f"{ef['game_n_examples'].tolist()}, reserve + give moves {give}, passes {npass}, {size} bytes")


if __name__ == "__main__":
    main()
