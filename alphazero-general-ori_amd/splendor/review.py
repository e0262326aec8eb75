"""Game review (the reference's review.py / analyze.py): search every position of recorded
games with a large budget and report, per turn, the value, the policy entropy, the candidate
lines and how the played move compares with the search's choice.

    rec = pit.record()                                   # BatchedArena / BatchedPit, after playGames
    rep = replay(engine, rec)                            # every position, rebuilt on the device
    out = review(game, evaluator, rec, dict(numMCTSSims=1600, cpuct=2.5, fpu=0.3))

All positions of all recorded games are independent roots: review() searches them as batches
of one BatchedMCTS, and reads the lines below the root with BatchedMCTS.principal_variations (a
read-only walk; re-rooting a handle to look deeper would collect the rest of its tree).
The post-processing (rank_moves, entropy, summarise) is numpy only.
"""
import numpy as np

PASS = 408
DEAL_STREAM = 0xFFFFFFFF
Q_UNSET = -42.0

RECORD_KEYS = ("game", "one_vs_two", "result", "plies", "score", "actions", "seed", "game_base", "n", "rules",
               "token_limit")


# ------------------------------------------------------------------ numpy post-processing
def rank_moves(counts):
    """counts int [..., A] -> the actions ordered by (visits descending, action ascending),
    int64 [..., A]: order[..., 0] is the most visited action, ties go to the lower action, and
    all-zero counts give 0, 1, 2, ..."""
    counts = np.asarray(counts)
    return np.argsort(-counts.astype(np.int64), axis=-1, kind="stable")


def entropy(probs):
    """Shannon entropy (nats) of each row of probs [..., A]; zero entries contribute nothing,
    so an all-zero row (a position that was not searched) gives 0."""
    p = np.asarray(probs, dtype=np.float64)
    logp = np.log(np.where(p > 0, p, 1.0))
    return np.maximum(-(p * logp).sum(-1), 0.0)


def summarise(counts, qsa, probs, value, played):
    """Per-position summary of N searched roots.
    counts int [N, A] root visit counts, qsa f64 [N, A] (-42 = unvisited), probs f64 [N, A],
    value f64 [N] the root value for the mover, played int [N] the move that was played.
    -> dict of [N] arrays: value, entropy, visits (total), best (the first action of
    rank_moves), best_visits, best_share, best_q, played, played_visits, played_share,
    played_rank (0 = the search's choice), played_q, q_loss = best_q - played_q where both
    edges have visits, else NaN (played_q / best_q are NaN for an unvisited edge; the shares
    are 0 when nothing was visited)."""
    counts = np.asarray(counts).astype(np.int64)
    qsa = np.asarray(qsa, dtype=np.float64)
    played = np.asarray(played).astype(np.int64)
    N = counts.shape[0]
    rows = np.arange(N)
    order = rank_moves(counts)
    best = order[:, 0] if N else np.zeros(0, np.int64)
    total = counts.sum(-1)
    rank = np.argmax(order == played[:, None], axis=-1) if N else np.zeros(0, np.int64)
    bv, pv = counts[rows, best], counts[rows, played]
    bq = np.where(bv > 0, qsa[rows, best], np.nan)
    pq = np.where(pv > 0, qsa[rows, played], np.nan)
    share = 1.0 / np.maximum(total, 1)
    return {"value": np.asarray(value, dtype=np.float64).reshape(N), "entropy": entropy(probs).reshape(N),
            "visits": total, "best": best, "best_visits": bv, "best_share": bv * share, "best_q": bq,
            "played": played, "played_visits": pv, "played_share": pv * share, "played_rank": rank,
            "played_q": pq, "q_loss": bq - pq}


# ------------------------------------------------------------------ replay
def _runs(ids):
    """Split positions 0..len(ids) into maximal runs of consecutive game ids."""
    out, s = [], 0
    for i in range(1, len(ids) + 1):
        if i == len(ids) or ids[i] != ids[i - 1] + 1:
            out.append((s, i))
            s = i
    return out


def replay(engine, record, games=None):
    """Rebuild every position of the chosen games (`games`: row indices of the record, default
    all) with the kernels that played them (BatchedArena._play_batch): the deal of game g is
    init(seed, DEAL_STREAM, board id game_base + g), ply p is step(action, player p % n,
    chance (seed, stream p, the same board id)) — the board id does not depend on the batch a
    game was played in. -> dict: boards int8 [G, P, R, 7] the real boards before each ply (P =
    the longest chosen game; zeros past a game's end), mover int8 [G, P], live bool [G, P]
    (ply < plies[g]), final int8 [G, R, 7] (device tensors), rows (the chosen record rows).
    Raises ValueError if the engine's players, rules or token limit are not the record's, or if
    the replay disagrees with the record: a recorded move that is not legal, a game that ends
    at another ply, another result (game_ended) or final score."""
    import torch
    from .env import ACTIONS, unpack_mask
    e, n, dev = engine, engine.n, engine.device
    if int(record["n"]) != n or int(record["rules"]) != e.rules or int(record["token_limit"]) != e.token_limit:
        raise ValueError(f"replay: the record was played with n={int(record['n'])}, rules={int(record['rules'])}, "
                         f"token_limit={int(record['token_limit'])}; the engine has n={n}, rules={e.rules}, "
                         f"token_limit={e.token_limit}")
    rows = np.arange(len(record["game"])) if games is None else np.asarray(games, dtype=np.int64).reshape(-1)
    gid = np.asarray(record["game"])[rows].astype(np.int64)
    plies = np.asarray(record["plies"])[rows].astype(np.int64)
    acts = np.asarray(record["actions"])[rows].astype(np.int16)
    if (plies <= 0).any() or (plies > acts.shape[1]).any():
        raise ValueError(f"replay: games {gid[(plies <= 0) | (plies > acts.shape[1])].tolist()} did not end in the record")
    seed, base = int(record["seed"]), int(record["game_base"])
    G, P = len(rows), int(plies.max()) if len(rows) else 0
    boards = torch.zeros((G, P, e.rows, 7), dtype=torch.int8, device=dev)
    final = e.new_state(G)
    mover = torch.from_numpy(np.tile((np.arange(P) % n).astype(np.int8), (G, 1))).to(dev)
    live = torch.from_numpy(np.arange(P)[None, :] < plies[:, None]).to(dev)
    for s0, s1 in _runs(gid):
        g, bid = s1 - s0, base + int(gid[s0])
        pl = torch.from_numpy(plies[s0:s1]).to(dev)
        want = torch.from_numpy(np.asarray(record["result"])[rows[s0:s1]].astype(np.float32)).to(dev)
        a_dev = torch.from_numpy(acts[s0:s1]).to(dev)
        st = e.new_state(g)
        e.init(st, None, seed=seed, stream=DEAL_STREAM, board_base=bid)
        for ply in range(int(plies[s0:s1].max())):
            on = pl > ply
            player = torch.full((g,), ply % n, dtype=torch.int8, device=dev)
            boards[s0:s1, ply] = st * on.to(torch.int8)[:, None, None]
            a = a_dev[:, ply]
            valid = unpack_mask(e.valid_moves(e.canonical(st, player)))
            ok = (a >= 0) & valid.gather(1, a.long().clamp(0, ACTIONS - 1).unsqueeze(1)).squeeze(1)
            if bool((on & ~ok).any()):
                bad = (on & ~ok).nonzero().flatten().cpu().numpy()
                raise ValueError(f"replay: games {gid[s0 + bad].tolist()}: the recorded move of ply {ply} is not legal")
            # (finished games idle on the no-op pass, as in the arena's loop)
            a = torch.where(on, a, torch.full_like(a, PASS))
            e.step(st, a, player=player, deterministic=False, seed=seed, stream=ply, board_base=bid)
            ended = e.game_ended(st)
            over = (ended != 0).any(1)
            last = pl == ply + 1
            if bool((on & (over != last)).any()):
                bad = (on & (over != last)).nonzero().flatten().cpu().numpy()
                raise ValueError(f"replay: games {gid[s0 + bad].tolist()} end at another ply than recorded "
                                 f"(ply {ply + 1})")
            if bool((last & (ended != want).any(1)).any()):
                bad = (last & (ended != want).any(1)).nonzero().flatten().cpu().numpy()
                raise ValueError(f"replay: games {gid[s0 + bad].tolist()}: the result differs from the record")
            final[s0:s1][last] = st[last]
    score = e.score(final).cpu().numpy() if G else np.zeros((0, n), np.int32)
    want = np.asarray(record["score"])[rows]
    if not np.array_equal(score, want):
        bad = np.flatnonzero((score != want).any(1))
        raise ValueError(f"replay: games {gid[bad].tolist()}: the final score differs from the record")
    return {"boards": boards, "mover": mover, "live": live, "final": final, "rows": rows}


# ------------------------------------------------------------------ review
def review(game, evaluator, record, args, games=None, lines=3, depth=8, batch=None, seed=0x5EED, mem_budget=None):
    """Search every live position of the chosen games (`games`: record rows, default all) as
    an independent root: the canonical form of each, in batches of `batch` trees (default:
    all positions, at most 4,096) of one BatchedMCTS(engine, batch, args, evaluator), every
    search full and from an empty tree; the last batch is padded with copies of its first
    position. -> dict with one row per live position, ordered by (record row, ply), numpy:
    row, game, ply, mover, scores int32 [N, n] (per seat), the columns of summarise() (value =
    the root value for the mover), and the lines of principal_variations(lines, depth) as
    pv_action / pv_visits / pv_q / pv_prior [N, lines, depth], pv_length / pv_end [N, lines];
    plus counts int64 [N, 409]."""
    import torch
    from .mcts import BatchedMCTS
    e = game.engine
    rep = replay(e, record, games)
    rows = rep["rows"]
    idx = rep["live"].nonzero()                             # [N, 2], (game, ply) ascending
    N = idx.shape[0]
    boards = rep["boards"][idx[:, 0], idx[:, 1]].contiguous()
    mover = rep["mover"][idx[:, 0], idx[:, 1]].contiguous()
    canon = e.canonical(boards, mover)
    gi, ply = idx[:, 0].cpu().numpy(), idx[:, 1].cpu().numpy()
    played = np.asarray(record["actions"])[rows][gi, ply].astype(np.int64)
    out = {"row": rows[gi], "game": np.asarray(record["game"])[rows][gi], "ply": ply,
           "mover": mover.cpu().numpy(), "scores": e.score(boards).cpu().numpy() if N else np.zeros((0, e.n), np.int32)}
    B = int(batch or min(max(N, 1), 4096))
    mcts = BatchedMCTS(e, B, args, evaluator=evaluator, dirichlet_noise=False, seed=seed, mem_budget=mem_budget)
    keep = {k: [] for k in ("counts", "qsa", "probs", "value", "action", "visits", "q", "prior", "length", "end")}
    for s in range(0, N, B):
        m = min(B, N - s)
        roots = canon[s:s + m]
        if m < B:
            roots = torch.cat([roots, roots[:1].expand(B - m, -1, -1)]).contiguous()
        probs, q, _, counts = mcts.get_action_prob(roots, force_full_search=True, keep_tree=False)
        pv = mcts.principal_variations(lines, depth)
        qsa = mcts.root_stats()[1]
        for k, t in (("counts", counts), ("qsa", qsa), ("probs", probs), ("value", q[:, 0])):
            keep[k].append(t[:m].cpu().numpy())
        for k in ("action", "visits", "q", "prior", "length", "end"):
            keep[k].append(pv[k][:m].cpu().numpy())
    if not N:
        return out
    cat = {k: np.concatenate(v) for k, v in keep.items()}
    out.update(summarise(cat["counts"], cat["qsa"], cat["probs"], cat["value"], played))
    out["counts"] = cat["counts"]
    for k in ("action", "visits", "q", "prior", "length", "end"):
        out["pv_" + k] = cat[k]
    return out


def evaluator_of(engine, spec, batch, seed=0x5EED):
    """The leaf evaluator of a pit player spec that searches (splendor.pit.MCTSPlayer,
    RolloutPlayer, MixedPlayer), built as BatchedPit seats it, for `batch` trees: the reviewer
    is any player the pit can rate."""
    from .pit import MCTSPlayer, MixedPlayer, RolloutPlayer
    from .playout import MixedEvaluator, PlayoutEvaluator
    from .search import evaluator_for
    if isinstance(spec, RolloutPlayer):
        return PlayoutEvaluator(engine, spec.playouts, spec.policy, seed=seed)
    if isinstance(spec, (MCTSPlayer, MixedPlayer)):
        ev = spec.evaluator
        if ev is None:
            ev = evaluator_for(engine, spec.nnet, batch, precision=spec.nn_precision)
        if isinstance(spec, MixedPlayer):
            ev = MixedEvaluator(engine, ev, spec.playouts, spec.policy, lam=spec.lam, seed=seed)
        return ev
    raise TypeError(f"a reviewer searches: expected MCTSPlayer, RolloutPlayer or MixedPlayer, got "
                    f"{type(spec).__name__}")


def line_string(actions, length, to_string=None):
    """The first `length` moves of one line as text (to_string: action -> str, default
    SplendorGame.move_to_str)."""
    if to_string is None:
        from .SplendorGame import move_to_str as to_string
    return "; ".join(to_string(int(a)) for a in list(actions)[:int(length)])
