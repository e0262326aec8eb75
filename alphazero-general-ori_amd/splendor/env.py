"""Batched, device-resident Splendor environment over libsplendor_amd.so.

Each method is one stream-ordered HIP launch over B boards held in HBM as torch tensors
(torch is only the allocator / stream provider here; all compute is the HIP engine).
Shapes follow the reference's per-board API, batched on a leading dimension:
    state  int8  [B, R, 7]   (SplendorLogicNumba.Board.state, :291-303)
    player int8  [B]
    mask   int64 [B, 7]      (409 legality bits, packed; unpack with `unpack_mask`)
"""
import ctypes as C

import torch

from . import _lib

ACTIONS = 409
MASK_WORDS = 7


def observation_rows(n_players):
    return 32 + 10 * n_players + n_players * n_players


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_BIT = None


def pack_mask(valid):
    """bool [...,409] -> [...,7] int64 packed words (bit i of word k = action 64k+i), the
    engine's mask layout; inverse of unpack_mask."""
    global _BIT
    if _BIT is None or _BIT.device != valid.device:
        _BIT = torch.arange(64, device=valid.device, dtype=torch.int64)
    pad = torch.zeros((*valid.shape[:-1], MASK_WORDS * 64), dtype=torch.int64, device=valid.device)
    pad[..., :ACTIONS] = valid.to(torch.int64)
    return (pad.view(*valid.shape[:-1], MASK_WORDS, 64) << _BIT).sum(-1)


def unpack_mask(mask):
    """[...,7] packed words -> bool [...,409] (on the same device)."""
    global _BIT
    if _BIT is None or _BIT.device != mask.device:
        _BIT = torch.arange(64, device=mask.device, dtype=torch.int64)
    bits = (mask.to(torch.int64).unsqueeze(-1) >> _BIT) & 1
    return bits.reshape(*mask.shape[:-1], MASK_WORDS * 64)[..., :ACTIONS].bool()


class SplendorEngine:
    """A rules context (players, token limit) bound to one device."""

    def __init__(self, n_players=2, token_limit=10, device="cuda"):
        self.L = _lib.lib()
        self.n = int(n_players)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NativeEngineMissing("the Splendor engine runs on a HIP device only")
        h = C.c_void_p()
        _lib.check(self.L.spl_ctx_create(self.n, int(token_limit), C.byref(h)), "spl_ctx_create")
        self.ctx = h
        self.token_limit = int(token_limit)
        self.rows = observation_rows(self.n)
        self.S = 7 * self.rows

    def __del__(self):
        if getattr(self, "ctx", None) is not None:
            self.L.spl_ctx_destroy(self.ctx)
            self.ctx = None

    # ------------------------------------------------------------- allocation helpers
    def new_state(self, B):
        return torch.zeros((B, self.rows, 7), dtype=torch.int8, device=self.device)

    def _s(self):
        return _stream(self.device)

    @staticmethod
    def _chance(uniforms):
        if uniforms is None:
            return None, 0
        assert uniforms.dtype == torch.float64 and uniforms.dim() == 2 and uniforms.is_contiguous()
        return _ptr(uniforms), uniforms.shape[1]

    # ------------------------------------------------------------- Game API, batched
    def init(self, state, player=None, seed=0, stream=0xFFFFFFFF, board_base=0, uniforms=None):
        """Board.init_game on every board (getInitBoard)."""
        up, us = self._chance(uniforms)
        _lib.check(self.L.spl_init(self.ctx, state.shape[0], _ptr(state), _ptr(player), up, us,
                                   seed, stream, board_base, self._s()), "spl_init")
        return state

    def valid_moves(self, state, player=None, out=None):
        B = state.shape[0]
        out = out if out is not None else torch.empty((B, MASK_WORDS), dtype=torch.int64, device=self.device)
        _lib.check(self.L.spl_valid_moves(self.ctx, B, _ptr(state), _ptr(player), _ptr(out), self._s()),
                   "spl_valid_moves")
        return out

    def step(self, state, action, player=None, next_player=None, deterministic=False, seed=0,
             stream=0, board_base=0, uniforms=None, err=None):
        """make_move in place (getNextState). action: int16 [B]."""
        B = state.shape[0]
        up, us = self._chance(uniforms)
        _lib.check(self.L.spl_step(self.ctx, B, _ptr(state), _ptr(player), _ptr(action),
                                   _ptr(next_player), int(bool(deterministic)), up, us, seed, stream,
                                   board_base, _ptr(err), self._s()), "spl_step")
        return next_player

    def game_ended(self, state, out=None):
        B = state.shape[0]
        out = out if out is not None else torch.empty((B, self.n), dtype=torch.float32, device=self.device)
        _lib.check(self.L.spl_game_ended(self.ctx, B, _ptr(state), _ptr(out), self._s()), "spl_game_ended")
        return out

    def canonical(self, state, player, out=None):
        out = out if out is not None else torch.empty_like(state)
        _lib.check(self.L.spl_canonical(self.ctx, state.shape[0], _ptr(state), _ptr(player), _ptr(out),
                                        self._s()), "spl_canonical")
        return out

    def score(self, state):
        out = torch.empty((state.shape[0], self.n), dtype=torch.int32, device=self.device)
        _lib.check(self.L.spl_score(self.ctx, state.shape[0], _ptr(state), _ptr(out), self._s()), "spl_score")
        return out

    def round(self, state):
        out = torch.empty((state.shape[0],), dtype=torch.int32, device=self.device)
        _lib.check(self.L.spl_round(self.ctx, state.shape[0], _ptr(state), _ptr(out), self._s()), "spl_round")
        return out

    def tree_step(self, parent, action, child=None, err=None):
        child = child if child is not None else torch.empty_like(parent)
        _lib.check(self.L.spl_tree_step(self.ctx, parent.shape[0], _ptr(parent), _ptr(action), _ptr(child),
                                        _ptr(err), self._s()), "spl_tree_step")
        return child

    def player_move(self, state, kind, active=None, pi=None, seed=0, stream=0, board_base=0, out=None,
                    cand_out=None, best_out=None):
        """One move of a rule-based player (_lib.PLAYER_RANDOM / _GREEDY / _POLICY;
        SplendorPlayers.py:18-25, :93-115) on each canonical board -> int16 [B]. active (uint8
        [B], optional): rows with 0 are skipped and keep their entries of every output. pi
        (f32 [B,409]): the POLICY player's priors. The choice among a board's candidates is the
        Philox draw (seed, board_base + b, stream). cand_out (int64 [B,7]) receives the packed
        candidate sets, best_out (int32 [B]) GREEDY's best score after one move."""
        B = state.shape[0]
        out = out if out is not None else torch.full((B,), -1, dtype=torch.int16, device=self.device)
        if pi is not None and (pi.dtype != torch.float32 or tuple(pi.shape) != (B, ACTIONS) or
                               not pi.is_contiguous()):
            raise ValueError(f"player_move: pi must be a contiguous f32 tensor of shape ({B}, {ACTIONS})")
        _lib.check(self.L.spl_player_move(self.ctx, B, _ptr(state), _ptr(active), int(kind), _ptr(pi), seed,
                                          int(stream), int(board_base), _ptr(out), _ptr(cand_out),
                                          _ptr(best_out), self._s()), "spl_player_move")
        return out

    def set_token_limit(self, n):
        """Board.setNumTokenLim (SplendorLogicNumba.py:214-215)."""
        _lib.check(self.L.spl_ctx_set_token_limit(self.ctx, int(n)), "spl_ctx_set_token_limit")
        self.token_limit = int(n)

    @property
    def rules(self):
        """The context's rule flags (_lib.RULE_*; 0 = the full game)."""
        r = int(self.L.spl_ctx_rules(self.ctx))
        _lib.check(min(r, 0), "spl_ctx_rules")
        return r

    def set_rules(self, no_reserve=False, flags=None):
        """Rule switches of every later call that builds a legality mask on this engine
        (valid_moves, player_move, rollouts, playouts) and of search handles created from now
        on; a BatchedMCTS keeps the rules it was created under. no_reserve: the reference's
        ENABLE_ACTION_RESERVE = False (SplendorGame.disableReserve): actions 12..26 are never
        legal, reserve + give (290..364) and everything else is unchanged. `flags` sets the
        raw word (what `rules` returns) instead. The token limit is untouched."""
        word = int(flags) if flags is not None else (_lib.RULE_NO_RESERVE if no_reserve else 0)
        _lib.check(self.L.spl_ctx_set_rules(self.ctx, word), "spl_ctx_set_rules")

    def symmetries(self, state, pi, valid):
        """Board.get_symmetries for E examples -> (state [E,K,R,7], pi [E,K,409],
        valid [E,K,7], present [E,K]) with K = 10 + 2n (reference order)."""
        E, K = state.shape[0], 10 + 2 * self.n
        dev = self.device
        os_ = torch.empty((E, K, self.rows, 7), dtype=torch.int8, device=dev)
        op = torch.empty((E, K, ACTIONS), dtype=torch.float32, device=dev)
        ov = torch.empty((E, K, MASK_WORDS), dtype=torch.int64, device=dev)
        pr = torch.empty((E, K), dtype=torch.uint8, device=dev)
        _lib.check(self.L.spl_symmetries(self.ctx, E, _ptr(state), _ptr(pi.contiguous()), _ptr(valid.contiguous()),
                                         _ptr(os_), _ptr(op), _ptr(ov), _ptr(pr), self._s()), "spl_symmetries")
        return os_, op, ov, pr

    def symmetry_counts(self, state):
        """Number of variants Board.get_symmetries emits for each of E boards -> uint8 [E]."""
        E = state.shape[0]
        out = torch.empty((E,), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.spl_symmetry_counts(self.ctx, E, _ptr(state.contiguous()), _ptr(out), self._s()),
                   "spl_symmetry_counts")
        return out

    def check_example_columns(self, state, pi, valid, winner, scdiff):
        """Raise unless the five example columns are what spl_gather_examples reads: contiguous
        device tensors of the ABI's types, one row per example."""
        E, n = state.shape[0], self.n
        for t, dt, shape in ((state, torch.int8, (E, self.rows, 7)), (pi, torch.float32, (E, ACTIONS)),
                             (valid, torch.int64, (E, MASK_WORDS)), (winner, torch.float32, (E, n)),
                             (scdiff, torch.int32, (E, n))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"example column: need a contiguous device {dt} tensor of shape {shape}")

    def gather_examples(self, state, pi, valid, winner, scdiff, example, ordinal, err=None, rows=None,
                        check=True):
        """Training rows from unexpanded example columns in one launch: row i is variant
        number ordinal[i] (int32, among the variants get_symmetries emits, in its order) of
        example example[i] (int64). -> (x f32 [M,R,7], pi f32 [M,409], valid bool [M,409],
        winner f32 [M,n], scdiff int32 [M,n]). Nothing is allocated or synchronised beyond
        the outputs; rows with an index out of range come back as zeros and set
        _lib.ERR_BAD_INDEX in `err` (device int32, optional). `rows` (default: all of
        `state`) is the number of examples E; check=False skips check_example_columns for
        columns the caller has checked already."""
        E = int(state.shape[0] if rows is None else rows)
        M, dev, n = int(example.shape[0]), self.device, self.n
        if check:
            self.check_example_columns(state, pi, valid, winner, scdiff)
        if example.dtype != torch.int64 or ordinal.dtype != torch.int32 or not example.is_cuda or \
                not ordinal.is_cuda or not example.is_contiguous() or not ordinal.is_contiguous():
            raise ValueError("gather_examples: example int64 / ordinal int32 contiguous device tensors")
        if example.shape != (M,) or ordinal.shape != (M,) or E > state.shape[0] or (M and not E):
            raise ValueError("gather_examples: example / ordinal / column sizes disagree")
        x = torch.empty((M, self.rows, 7), dtype=torch.float32, device=dev)
        op = torch.empty((M, ACTIONS), dtype=torch.float32, device=dev)
        ov = torch.empty((M, ACTIONS), dtype=torch.bool, device=dev)
        ow = torch.empty((M, n), dtype=torch.float32, device=dev)
        osd = torch.empty((M, n), dtype=torch.int32, device=dev)
        _lib.check(self.L.spl_gather_examples(self.ctx, E, M, _ptr(state), _ptr(pi), _ptr(valid), _ptr(winner),
                                              _ptr(scdiff), _ptr(example), _ptr(ordinal), _ptr(x), _ptr(op),
                                              _ptr(ov), _ptr(ow), _ptr(osd), _ptr(err), self._s()),
                   "spl_gather_examples")
        return x, op, ov, ow, osd

    def rollout_step(self, state, player, mask_out, action_out, ended_out, games_done, seed, step,
                     board_base=0):
        _lib.check(self.L.spl_rollout_step(self.ctx, state.shape[0], _ptr(state), _ptr(player),
                                           _ptr(mask_out), _ptr(action_out), _ptr(ended_out),
                                           _ptr(games_done), seed, step, board_base, self._s()),
                   "spl_rollout_step")

    def rollout_run(self, K, state, player, mask_out, action_out, ended_out, games_done, seed, step0,
                    board_base=0):
        """K fused moves in one launch; outputs stacked by move ([K][B]...)."""
        _lib.check(self.L.spl_rollout_run(self.ctx, state.shape[0], int(K), _ptr(state), _ptr(player),
                                          _ptr(mask_out), _ptr(action_out), _ptr(ended_out),
                                          _ptr(games_done), seed, step0, board_base, self._s()),
                   "spl_rollout_run")

    PLAYOUT_POLICIES = {"uniform": _lib.PLAYOUT_UNIFORM, "buy_first": _lib.PLAYOUT_BUY_FIRST}

    def playout(self, state, player=None, active=None, policy="buy_first", playouts=1, max_steps=None,
                seed=0, step0=0, board_base=0, pi=False, steps=False, out=None):
        """`playouts` random playouts of every board to the end of its game in one launch
        (spl_playout) -> {"result": f32 [B,n] mean outcome in the input board's seat order,
        "unfinished": int32 [1] playouts cut off by max_steps (default 62 n: none), "pi": f32
        [B,409] uniform prior over the legal moves (pi=True), "steps": int32 [B,playouts]
        moves played (steps=True)}. player (int8 [B], default 0) is each board's mover; rows
        with active[b] == 0 (uint8 [B]) run nothing and keep their entries of every output.
        policy: "uniform" or "buy_first" (or the _lib.PLAYOUT_* code). Playout j of row b
        draws from Philox (seed, board_base + b playouts + j), streams step0, step0 + 1, ..
        `out`: a dict from an earlier call whose tensors are reused."""
        B, P, dev = state.shape[0], int(playouts), self.device
        kind = self.PLAYOUT_POLICIES.get(policy, policy)
        if not isinstance(kind, int):
            raise ValueError(f"playout: policy must be one of {sorted(self.PLAYOUT_POLICIES)}, got {policy!r}")
        for t, dt, name in ((state, torch.int8, "state"), (player, torch.int8, "player"), (active, torch.uint8, "active")):
            if t is not None and (t.dtype != dt or t.shape[0] != B or not t.is_contiguous()):
                raise ValueError(f"playout: {name} must be a contiguous {dt} tensor with {B} rows")
        out = dict(out) if out is not None else {}
        if "result" not in out:
            out["result"] = torch.zeros((B, self.n), dtype=torch.float32, device=dev)
        if pi and "pi" not in out:
            out["pi"] = torch.zeros((B, ACTIONS), dtype=torch.float32, device=dev)
        if steps and "steps" not in out:
            out["steps"] = torch.zeros((B, P), dtype=torch.int32, device=dev)
        if "unfinished" not in out:                              # (a reused counter keeps adding up)
            out["unfinished"] = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.L.spl_playout(self.ctx, B, _ptr(state), _ptr(player), _ptr(active), kind, P,
                                      int(62 * self.n if max_steps is None else max_steps), seed, int(step0),
                                      int(board_base), _ptr(out["result"]), _ptr(out["pi"]) if pi else None,
                                      _ptr(out["steps"]) if steps else None, _ptr(out["unfinished"]), self._s()),
                   "spl_playout")
        return out

    def playout_seq(self, state, call_seq, active=None, index=None, count=None, policy="buy_first", playouts=1,
                    max_steps=None, seed=0, board_base=0, pi=False, steps=False, out=None):
        """playout() for the search's leaves, safe to capture in a graph (spl_playout_seq): the
        boards are canonical (mover = seat 0) and the stream base is read on the device, step0 =
        (call_seq[0] mod 2^23) 256 with call_seq a one-element device tensor of 4-byte integers
        that the launch only reads (the caller advances it on the stream). The rows that run:
        the leaf list index / count (int32 [B] / [ceil(B / 64)], as spl_mcts_select_compact
        writes it) if given, else the rows with active[b] != 0, else all; every other row keeps
        its entries of every output. Results, bit for bit, as playout(active = those rows,
        step0 = that base). max_steps is at most 256."""
        B, P, dev = state.shape[0], int(playouts), self.device
        kind = self.PLAYOUT_POLICIES.get(policy, policy)
        if not isinstance(kind, int):
            raise ValueError(f"playout_seq: policy must be one of {sorted(self.PLAYOUT_POLICIES)}, got {policy!r}")
        for t, dt, rows, name in ((state, (torch.int8,), B, "state"), (active, (torch.uint8,), B, "active"),
                                  (index, (torch.int32,), B, "index"), (count, (torch.int32,), (B + 63) // 64, "count"),
                                  (call_seq, (torch.int32, torch.uint32), 1, "call_seq")):
            if t is not None and (t.dtype not in dt or t.shape[0] != rows or not t.is_contiguous()):
                raise ValueError(f"playout_seq: {name} must be a contiguous {dt[0]} tensor with {rows} rows")
        if call_seq is None or (index is None) != (count is None) or (active is not None and index is not None):
            raise ValueError("playout_seq: call_seq is required; index and count go together and exclude active")
        out = dict(out) if out is not None else {}
        if "result" not in out:
            out["result"] = torch.zeros((B, self.n), dtype=torch.float32, device=dev)
        if pi and "pi" not in out:
            out["pi"] = torch.zeros((B, ACTIONS), dtype=torch.float32, device=dev)
        if steps and "steps" not in out:
            out["steps"] = torch.zeros((B, P), dtype=torch.int32, device=dev)
        if "unfinished" not in out:                              # (a reused counter keeps adding up)
            out["unfinished"] = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.L.spl_playout_seq(self.ctx, B, _ptr(state), _ptr(active), _ptr(index), _ptr(count), kind, P,
                                          int(62 * self.n if max_steps is None else max_steps), seed, _ptr(call_seq),
                                          int(board_base), _ptr(out["result"]), _ptr(out["pi"]) if pi else None,
                                          _ptr(out["steps"]) if steps else None, _ptr(out["unfinished"]), self._s()),
                   "spl_playout_seq")
        return out

    def playout_mix(self, state, call_seq, lam, v, active=None, index=None, count=None, policy="buy_first",
                    playouts=1, max_steps=None, seed=0, board_base=0, unfinished=None):
        """playout_seq() blended into a value buffer (spl_playout_mix): for every row that runs,
        v[b] = (1 - l) v[b] + l mean[b] in f32, in place, with the rows, the keys and the mean of
        playout_seq(call_seq, ...). lam is a one-element f32 device tensor read on the device and
        clamped to 0..1 there (NaN counts as 0), so a write to it reaches a captured launch; at 0
        the launch changes nothing. v: f32 [B, n], contiguous (the network's values). Rows that do
        not run keep every byte of v. Returns (v, unfinished), the counter an int32 [1] that
        accumulates (`unfinished`: one from an earlier call)."""
        B, P, dev = state.shape[0], int(playouts), self.device
        kind = self.PLAYOUT_POLICIES.get(policy, policy)
        if not isinstance(kind, int):
            raise ValueError(f"playout_mix: policy must be one of {sorted(self.PLAYOUT_POLICIES)}, got {policy!r}")
        for t, dt, rows, name in ((state, (torch.int8,), B, "state"), (active, (torch.uint8,), B, "active"),
                                  (index, (torch.int32,), B, "index"), (count, (torch.int32,), (B + 63) // 64, "count"),
                                  (call_seq, (torch.int32, torch.uint32), 1, "call_seq"),
                                  (lam, (torch.float32,), 1, "lam"), (v, (torch.float32,), B, "v")):
            if t is not None and (t.dtype not in dt or t.shape[0] != rows or not t.is_contiguous()):
                raise ValueError(f"playout_mix: {name} must be a contiguous {dt[0]} tensor with {rows} rows")
        if call_seq is None or lam is None or v is None or tuple(v.shape) != (B, self.n):
            raise ValueError(f"playout_mix: call_seq, lam and v (f32 [{B}, {self.n}]) are required")
        if (index is None) != (count is None) or (active is not None and index is not None):
            raise ValueError("playout_mix: index and count go together and exclude active")
        if unfinished is None:
            unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.L.spl_playout_mix(self.ctx, B, _ptr(state), _ptr(active), _ptr(index), _ptr(count), kind, P,
                                          int(62 * self.n if max_steps is None else max_steps), seed, _ptr(call_seq),
                                          int(board_base), _ptr(lam), _ptr(v), _ptr(unfinished), self._s()),
                   "spl_playout_mix")
        return v, unfinished


class RolloutBatch:
    """B boards of random-policy self-play, stepped by one fused launch per step
    (BASELINE config 2). All buffers live in HBM for the whole run."""

    def __init__(self, engine, B, seed=0x5EED, board_base=0):
        self.e = engine
        self.B = B
        self.seed = seed
        self.board_base = board_base
        dev = engine.device
        self.state = engine.new_state(B)
        self.player = torch.zeros(B, dtype=torch.int8, device=dev)
        self.mask = torch.zeros((B, MASK_WORDS), dtype=torch.int64, device=dev)
        self.action = torch.zeros(B, dtype=torch.int16, device=dev)
        self.ended = torch.zeros((B, engine.n), dtype=torch.float32, device=dev)
        self.games = torch.zeros(B, dtype=torch.int32, device=dev)
        self.t = 0
        engine.init(self.state, self.player, seed=seed, stream=0xFFFFFFFF, board_base=board_base)

    def step(self):
        self.e.rollout_step(self.state, self.player, self.mask, self.action, self.ended, self.games,
                            self.seed, self.t, self.board_base)
        self.t += 1

    def launcher(self, K, out):
        """A prebuilt launch of `run(K, out=out)`: every argument but the step counter is
        converted once, so a timed region pays one ctypes call per launch (bench.py)."""
        e = self.e
        fn = e.L.spl_rollout_run
        head = (e.ctx, self.B, int(K), _ptr(self.state), _ptr(self.player), _ptr(out["mask"]),
                _ptr(out["action"]), _ptr(out["ended"]), _ptr(self.games), self.seed)
        tail = (self.board_base, e._s())

        def launch():
            rc = fn(*head, self.t, *tail)
            if rc:
                _lib.check(rc, "spl_rollout_run")
            self.t += K
        return launch

    def run(self, K, masks=True, out=None):
        """K moves in one launch (boards stay on chip); returns the stacked per-move outputs
        {"mask": [K,B,7] or None, "action": [K,B], "ended": [K,B,n]} (reused if `out`)."""
        B, dev, n = self.B, self.e.device, self.e.n
        if out is None or out["action"].shape[0] != K:
            out = {"mask": torch.empty((K, B, MASK_WORDS), dtype=torch.int64, device=dev) if masks else None,
                   "action": torch.empty((K, B), dtype=torch.int16, device=dev),
                   "ended": torch.empty((K, B, n), dtype=torch.float32, device=dev)}
        self.e.rollout_run(K, self.state, self.player, out["mask"], out["action"], out["ended"], self.games,
                           self.seed, self.t, self.board_base)
        self.t += K
        return out
