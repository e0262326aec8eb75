// splendor_env.hip — batched Splendor environment kernels for gfx950 + the C ABI
// declared in include/splendor_amd.h.
//
// Mapping: one 64-lane wave per board, 4 boards per 256-thread workgroup; each wave stages
// its board in its own LDS slot (Lay<N>::LS bytes, 8-byte rows), so boards never share LDS
// and no workgroup barrier is needed (waves exit independently). The fused rollout kernel
// instead owns 64 boards per workgroup (see k_rollout). Device logic: splendor_device.h.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/splendor_amd.h"

#ifndef ROLLOUT_ABLATE
#define ROLLOUT_ABLATE 0   // diagnostic builds only (tools/ablate_rollout.hip): 1 = skip mask, 2 = skip move
#endif
#ifndef ROLLOUT_PRIO
#define ROLLOUT_PRIO 1     // k_rollout: raise the wave priority of each phase's longest pipeline (0 = off, A/B)
#endif
#ifndef ROLLOUT_TIMING
#define ROLLOUT_TIMING 0   // diagnostic builds only (tools/time_rollout.hip): per-block cycle totals
#endif
#if ROLLOUT_TIMING
// block-shared cycle accumulators; SPL_PROBE(k) charges the cycles since the previous probe
// to slot k (thread 0's view; in product builds SPL_PROBE expands to nothing)
__shared__ uint64_t spl_probe_acc[32];
__shared__ uint64_t spl_probe_last;
#define SPL_PROBE(k)                                                                       \
    if (threadIdx.x == 0) {                                                                \
        const uint64_t c_ = clock64();                                                     \
        spl_probe_acc[k] += c_ - spl_probe_last;                                           \
        spl_probe_last = c_;                                                               \
    }
__device__ uint64_t *g_rollout_timing;
#endif
#include "board_phases.h"
#include "mcts_device.h"   // ST_PLAYER
#include "spl_ctx.h"

using namespace spl;

namespace {

constexpr int WAVES = 4;            // boards per workgroup
constexpr int THREADS = 64 * WAVES;

// ---------------------------------------------------------------- kernels
template <int N>
__global__ __launch_bounds__(THREADS) void k_init(int B, int8_t *__restrict__ state,
                                                  int8_t *__restrict__ player,
                                                  const double *__restrict__ u, int ustride,
                                                  uint64_t seed, uint32_t stream, uint32_t bbase) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][Lx::LS];
    __shared__ double ub[WAVES][DEAL_DRAWS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    int8_t *s = lds[w];
    const double *du = u ? u + (size_t)b * ustride : ub[w];
    if (!u) wave_philox_uniforms(ub[w], seed, bbase + (uint32_t)b, stream, 0, DEAL_DRAWS);
    wave_init_game<N>(s, du);
    wave_store_board<N>(state + (size_t)b * Lx::S, s);
    if (player && lane_id() == 0) player[b] = 0;
}

template <int N>
__global__ __launch_bounds__(THREADS) void k_valid(int B, const int8_t *__restrict__ state,
                                                   const int8_t *__restrict__ player, int lim,
                                                   uint64_t *__restrict__ mask) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][Lx::LS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    int8_t *s = lds[w];
    wave_load_board<N>(s, state + (size_t)b * Lx::S);
    const int p = player ? player[b] : 0;
    uint64_t m[7];
    wave_valid_moves<N>(s, p, lim, m);
    store_mask(mask + (size_t)b * 7, m);
}

template <int N>
__global__ __launch_bounds__(THREADS) void k_step(int B, int8_t *__restrict__ state,
                                                  const int8_t *__restrict__ player,
                                                  const int16_t *__restrict__ action,
                                                  int8_t *__restrict__ next_player, int det,
                                                  const double *__restrict__ u, int ustride,
                                                  uint64_t seed, uint32_t stream, uint32_t bbase,
                                                  int32_t *err) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][Lx::LS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    const int a = action[b];
    const int p = player ? player[b] : 0;
    if (a < 0 || a >= SPL_ACTIONS) {
        if (err && lane_id() == 0) atomicOr(err, SPL_ERR_BAD_ACTION);
        if (next_player && lane_id() == 0) next_player[b] = (int8_t)p;
        return;
    }
    int8_t *s = lds[w];
    int8_t *g = state + (size_t)b * Lx::S;
    wave_load_board<N>(s, g);
    Chance ch{u ? u + (size_t)b * ustride : nullptr, seed, bbase + (uint32_t)b, stream, 0};
    const int nxt = make_move<N>(s, a, p, det != 0, ch);
    __builtin_amdgcn_wave_barrier();
    wave_store_board<N>(g, s);
    if (next_player && lane_id() == 0) next_player[b] = (int8_t)nxt;
}

// end / score / round read ~20 bytes per board: one lane per board straight from HBM
template <int N>
__global__ __launch_bounds__(256) void k_ended(int B, const int8_t *__restrict__ state,
                                               float *__restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float e[N];
    check_end_rows<N>(HbmRows{state + (size_t)b * Lay<N>::S}, e);
#pragma unroll
    for (int i = 0; i < N; i++) out[(size_t)b * N + i] = e[i];
}

template <int N>
__global__ __launch_bounds__(256) void k_score_round(int B, const int8_t *__restrict__ state,
                                                     int32_t *__restrict__ score,
                                                     int32_t *__restrict__ round) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int8_t *s = state + (size_t)b * Lay<N>::S;
    if (score)
#pragma unroll
        for (int p = 0; p < N; p++) score[(size_t)b * N + p] = score_rows<N>(HbmRows{s}, p);
    if (round) round[b] = (uint8_t)s[6];
}

template <int N>
__global__ __launch_bounds__(THREADS) void k_canonical(int B, const int8_t *__restrict__ state,
                                                       const int8_t *__restrict__ player,
                                                       int8_t *out) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][Lx::LS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    int8_t *s = lds[w];
    wave_load_board<N>(s, state + (size_t)b * Lx::S);
    const int p = player ? player[b] : 0;
    if (p) wave_roll_players<N>(s, s, p);
    wave_store_board<N>(out + (size_t)b * Lx::S, s);
}

template <int N>
__global__ __launch_bounds__(THREADS) void k_tree_step(int B, const int8_t *__restrict__ parent,
                                                       const int16_t *__restrict__ action,
                                                       int8_t *__restrict__ child, int32_t *err) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][Lx::LS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    int8_t *s = lds[w];
    wave_load_board<N>(s, parent + (size_t)b * Lx::S);
    const int a = action[b];
    if (a < 0 || a >= SPL_ACTIONS) {
        if (err && lane_id() == 0) atomicOr(err, SPL_ERR_BAD_ACTION);
    } else {
        Chance ch{nullptr, 0, 0, 0, 0};
        const int nxt = make_move<N>(s, a, 0, true, ch);
        __builtin_amdgcn_wave_barrier();
        if (nxt) wave_roll_players<N>(s, s, nxt);
    }
    wave_store_board<N>(child + (size_t)b * Lx::S, s);
}

// The rule-based players (splendor_amd.h spl_player_move): one move of a random, greedy or
// arg-max-policy player on each canonical board, wave per board. The candidate set is built
// as a packed mask from the legality mask; one keyed draw picks among its bits.
// Greedy lookahead: only buys (0-11 visible, 27-29 reserved) change a score and a score
// never falls, so every other legal move scores s0 and at most 15 moves are tried, each by
// the engine's make_move (deterministic) on a scratch copy in the wave's second LDS slot.
template <int N>
__global__ __launch_bounds__(THREADS) void k_player_move(int B, const int8_t *__restrict__ state,
                                                         const uint8_t *__restrict__ active, int kind,
                                                         const float *__restrict__ pi, int lim,
                                                         uint64_t seed, uint32_t stream, uint32_t bbase,
                                                         int16_t *__restrict__ action,
                                                         uint64_t *__restrict__ cand_out,
                                                         int32_t *__restrict__ best_out) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][2][Lx::LS];
    const int w = threadIdx.x >> 6, b = blockIdx.x * WAVES + w;
    if (b >= B) return;
    if (active && !active[b]) return;
    const int l = lane_id();
    int8_t *s = lds[w][0], *t = lds[w][1];
    wave_load_board<N>(s, state + (size_t)b * Lx::S);
    uint64_t v[7], c[7];
    wave_valid_moves<N>(s, 0, lim, v);
#pragma unroll
    for (int k = 0; k < 7; k++) c[k] = v[k];
    const int s0 = get_score<N>(s, 0);
    int best = s0;
    if (kind == SPL_PLAYER_GREEDY) {
        uint64_t top = 0;
        for (uint64_t r = uniform64(v[0] & 0x38000FFFull); r; r &= r - 1) {
            const int a = __ffsll((unsigned long long)r) - 1;
            wave_copy_lds_board<N>(t, s);
            Chance ch{nullptr, 0, 0, 0, 0};
            make_move<N>(t, a, 0, true, ch);
            __builtin_amdgcn_wave_barrier();
            const int sa = get_score<N>(t, 0);
            __builtin_amdgcn_wave_barrier();
            if (sa > best) {
                best = sa;
                top = 0;
            }
            if (sa == best) top |= 1ull << a;
        }
        const uint64_t vis = v[0] & 0xFFFull, gems = v[0] & 0x0FFFFFFFC0000000ull;   // [0,12), [30,60)
        const uint64_t first = best > s0 ? top : (vis ? vis : gems);
        if (first) {
            c[0] = first;
#pragma unroll
            for (int k = 1; k < 7; k++) c[k] = 0;
        }
    } else if (kind == SPL_PLAYER_POLICY) {
        const float *p = pi + (size_t)b * SPL_ACTIONS;
        float x[7], mx = 0.f;
        bool have = false;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const bool on = (v[k] >> l) & 1;                 // (bits >= 409 are never set)
            x[k] = on ? p[64 * k + l] : 0.f;
            if (on) mx = have ? fmaxf(mx, x[k]) : x[k];
            have |= on;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ox = __shfl_xor(mx, o, 64);
            const bool oh = __shfl_xor((int)have, o, 64);
            if (oh) mx = have ? fmaxf(mx, ox) : ox;
            have |= oh;
        }
        uint64_t any = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            c[k] = __ballot(((v[k] >> l) & 1) && x[k] == mx);
            any |= c[k];
        }
        if (!any) {                                          // (every legal entry NaN)
#pragma unroll
            for (int k = 0; k < 7; k++) c[k] = v[k];
        }
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) cnt += __popcll(c[k]);
    const double u = philox_u01(seed, bbase + (uint32_t)b, ST_PLAYER | stream, 0);
    const int a = select_bit(c, min((int)(u * (double)cnt), cnt - 1));
    if (l == 0) {
        action[b] = (int16_t)a;
        if (best_out) best_out[b] = best;
    }
    if (cand_out) store_mask(cand_out + (size_t)b * 7, c);
}

// Fused random-policy self-play (splendor_amd.h spl_rollout_step / spl_rollout_run).
// A 256-thread workgroup owns RB = 64 consecutive boards and keeps them in LDS, as 8-byte
// rows at an odd-qword stride (conflict-free lane-per-board ds_read_b64/ds_write_b64), for
// all K moves of the launch:
//   load     HBM -> LDS, one 4-row quad per thread (7 dwords -> 4 qwords), deck tables
//   per move t (step = step0 + t), four phases between LDS-only barriers:
//     preds  lane-per-board legality predicates on the real board for the player to move
//            (== the canonical form's mask: it only reads player p's rows), part w in wave
//            w (cards 0-5 / cards 6-11 / reserved cards, decks, conditions / colour
//            levels); wave 3 also draws Philox blocks 0-1 of every board's step stream
//            (draw 0 picks the action, 1-2 feed a deck draw)
//     mask   mask words w, w+4 in wave w (factorised words, lane_mask_word_fast)
//     select lane l < 16 of wave w = board 16w + l: pass bit (:263), uniform action draw;
//            boards filed by move kind
//     move   the masks go to HBM; wave k makes the moves of kind k (gem vectors / buy /
//            reserve / buy reserved), lane per board: chance, end check, per-move outputs;
//            then it re-deals the games its moves finished (wave-collective, draws 3..)
//   store    boards, players, game counters LDS -> HBM
#ifndef ROLLOUT_RB
#define ROLLOUT_RB 64
#endif
constexpr int RB = ROLLOUT_RB;   // boards per workgroup (<= 64: lane per board)
#define RT_MARK(k) SPL_PROBE(k)

template <int N>
__global__ __launch_bounds__(THREADS) void k_rollout(int B, int K, int8_t *__restrict__ state,
                                                     int8_t *__restrict__ player, int lim,
                                                     uint64_t *__restrict__ mask_out,
                                                     int16_t *__restrict__ action_out,
                                                     float *__restrict__ ended_out,
                                                     int32_t *__restrict__ games_done,
                                                     uint64_t seed, uint32_t step0, uint32_t bbase) {
    using Lx = Lay<N>;
    using Cv = Conv<N>;
    constexpr int ST = RolloutLds<N>::STRIDE;
    constexpr int PER = RB / WAVES;
    static_assert(PER * 4 == 64, "select: four lanes per board, one wave per PER boards");
    __shared__ __align__(16) int8_t lds[RB * ST];
    __shared__ uint64_t msk[RB][7];    // legality masks (odd qword stride: conflict-free)
    __shared__ int8_t pl[RB];
    __shared__ int32_t gdone[RB];
    __shared__ double ud[RB][4];       // draws 0..3 of each board's step stream
    __shared__ double ub[WAVES][DEAL_DRAWS];
    __shared__ TabsLds tabs;
    __shared__ uint64_t mfac[MASK_FACTOR_WORDS];
    __shared__ uint32_t klist[4][RB];  // per move kind (file_move)
    __shared__ int kcount[4];
    __shared__ PredLds<RB> pred;
    __shared__ DealRec drec[2][RB];     // deals of games gd0+1, gd0+2 of every board
    __shared__ int32_t gd0[RB];
    const int b0 = blockIdx.x * RB, nb = min(RB, B - b0);
    // the wave index in an SGPR: the per-wave choices of the shared phases (board_phases.h) are
    // scalar branches. As a vector value their compares stay in the move loop: 3 % slower on
    // the env benchmark, 1.3 % on playouts (profiles/shared_phases_ab.json).
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = lane_id();
    int8_t *const gst = state + (size_t)b0 * Lx::S;
#if ROLLOUT_TIMING
    if (tid < 32) spl_probe_acc[tid] = 0;
    if (tid == 0) spl_probe_last = clock64();
    const uint64_t wall0 = wall_clock64();
#endif
    // prologue: every global load (boards, players, game counters, the LDS tables) is issued
    // before the first LDS store. Strided copy loops waited one L2 / HBM round trip per
    // iteration: 13 of them, 15.5 K cycles of a 20-move launch's ~210 K (tools/time_rollout).
    {
        // (the deal tasks' game counters first: vmcnt retires loads in order, so the deals
        // below wait for these alone)
        int32_t gt[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int b = ((tid + j * THREADS) >> 2) % RB;
            gt[j] = games_done[b0 + min(b, nb - 1)];      // (never null: spl_rollout_run checks)
        }
        TabsRegs<THREADS> q_tabs;
        q_tabs.fetch(tid);
        const int bi = min(tid, nb - 1);
        const int8_t p0 = player[b0 + bi];
        const int32_t g0 = games_done[b0 + bi];
        BoardRegs<N, RB, THREADS> q_boards;
        q_boards.fetch(gst, nb, tid);
        // the next deals of every board (one for launches of 4-47 moves, two beyond),
        // computed up front by four lanes per deal (3 tiers + nobles, lane_deal_part) so that
        // ending a game costs a row expansion, not the draws; a game ending beyond them draws
        // its deal on the spot (same keys). They read the constant tables and their own game
        // counters, so they run while the loads above are in flight.
        const int pre = K >= 48 ? 2 : (K >= 4 ? 1 : 0);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int task = tid + j * THREADS, part = task & 3, rec = task >> 2, k = rec / RB, b = rec - k * RB;
            if (task < pre * RB * 4 && b < nb)
                lane_deal_part<N>(seed, bbase + (uint32_t)(b0 + b), (uint32_t)(gt[j] + 1 + k), part, Tabs{}, drec[k][b]);
        }
        q_boards.put(lds, gst, nb, tid);
        if (tid < nb) {
            pl[tid] = p0;
            gdone[tid] = g0;
            gd0[tid] = g0;
        }
        if (tid < 4) kcount[tid] = 0;
        q_tabs.put(tabs, mfac, tid);
    }
    const int pre = K >= 48 ? 2 : (K >= 4 ? 1 : 0);
    // every barrier of the move loop orders LDS only: the per-move outputs are write-only
    // HBM streams, and waiting for their stores (__syncthreads) cost ~2K cycles a barrier
    lds_sync();
    RT_MARK(0)
    for (int t = 0; t < K; t++) {
        const uint32_t step = step0 + (uint32_t)t;
        const size_t ob = (size_t)t * B + b0;            // this move's output row base
        if (tid < 4) kcount[tid] = 0;                    // (last read in the previous move phase)
        // draws 0-3 of every board's step stream, on wave 3 (its predicate part is the lightest)
        // wave priority: the SIMD's other waves (the co-resident workgroup's) yield issue
        // slots to the wave on this phase's critical path (predicate part 2; buy / reserve
        // moves below): 8.17 -> 8.7 G rollouts/s, tools/ab_rollout.sh
        if (ROLLOUT_PRIO && w == 2) __builtin_amdgcn_s_setprio(1);
        if (w == 3 && l < nb) {
#pragma unroll
            for (int k = 0; k < 2; k++)
                philox_pair(seed, bbase + (uint32_t)(b0 + l), step, k, ud[l][2 * k], ud[l][2 * k + 1]);
        }
        // predicates: wave w computes part w of every board's predicate set (lane per board)
        if (ROLLOUT_ABLATE != 1 && l < nb) phase_predicates<N>(w, l, lds + l * ST, pl[l], lim, pred);
        if (ROLLOUT_PRIO) __builtin_amdgcn_s_setprio(0);
        RT_MARK(16)
        lds_sync();
        RT_MARK(17)
        // mask words w and w+4 of every board: factorised words from the card predicates,
        // condition bits and colour levels; boards outside the fast domain take the exact
        // predicates and the per-action descriptor words
        if (ROLLOUT_ABLATE != 1 && l < nb) {
#if ROLLOUT_TIMING
            {   // diagnostic: waves that take the exact predicate path (slot 18), lanes (19)
                const uint64_t bm = __ballot(pred.any_bad(l));
                if (l == 0 && bm) { atomicAdd((unsigned long long *)&spl_probe_acc[18], 1ull);
                                    atomicAdd((unsigned long long *)&spl_probe_acc[19], (unsigned long long)__popcll(bm)); }
            }
#endif
            phase_mask_words<N>(w, l, lds + l * ST, pl[l], lim, pred, mfac, msk[l]);
        }
        lds_sync();
        RT_MARK(1)
        // select: four lanes per board (board w*16 + l/4; lane q = l%4 holds mask words 2q,
        // 2q+1), quad_select. Pass bit (:263) when nothing is legal; the board is filed by
        // move kind.
        {
            const int b = w * PER + (l >> 2), q = l & 3;
            const bool on = ROLLOUT_ABLATE != 2 && b < nb;
            uint64_t x0 = 0, x1 = 0;
            if (on) {
                x0 = msk[b][2 * q];
                if (q < 3) x1 = msk[b][2 * q + 1];
            }
            const QuadPick pk = quad_select(x0, x1, q, on ? ud[b][0] : 0.0);
            int a = pk.a;
            if (on) {
                if (ROLLOUT_ABLATE == 1) {
                    a = q == 0 ? 30 + (int)((step + b) % 5) : -1;
                } else if (pk.cnt == 0 && q == 3) {
                    a = 408;
                    x0 |= 1ull << (408 - 384);
                }
            }
            // the move's final mask goes to HBM from these registers (no LDS re-read)
            if (mask_out && on && ROLLOUT_ABLATE != 1) {
                uint64_t *mo = mask_out + (ob + b) * 7 + 2 * q;
                mo[0] = x0;
                if (q < 3) mo[1] = x1;
            }
            if (a >= 0) file_move(klist, kcount, b, a, pl[b]);
        }
        lds_sync();
        RT_MARK(5)
        // move phase. Wave w makes every move
        // of kind w (one pipeline specialisation per wave, so no wave carries the stages of
        // other kinds): chance draws 1-2, end check, outputs. Then the wave re-deals the games
        // its own moves finished (wave-collective; draws 3.. of the step stream) — mostly the
        // gem-move wave, which has the shortest pipeline, so the deals fill its wait for the
        // other kinds instead of taking a phase of their own.
#if ROLLOUT_TIMING
        const uint64_t mv0 = clock64();
#endif
        {
            int b = 0;
            bool ended = false;
            const int kc = kcount[w];
            const uint32_t ke = klist[w][l];                 // (read before the count is known)
            if (ROLLOUT_PRIO && (w == MK_BUY || w == MK_RESERVE)) __builtin_amdgcn_s_setprio(2);
            if (ROLLOUT_ABLATE != 2 && l < kc) {
                b = ke & 0xFF;
                const int a = (ke >> 8) & 0xFFF, p = ke >> 20;
                int8_t *s = lds + b * ST;
                int r;                                            // the round after the move
                int nxt = lane_move_of_kind<N>(w, s, a, p, &ud[b][0], tabs.view(), r);
                RT_MARK(6)
#if ROLLOUT_TIMING
                // per wave: move pipeline up to make_move's end (slots 28+w, lane 0's board)
                if (l == 0) atomicAdd((unsigned long long *)&spl_probe_acc[28 + w], (unsigned long long)(clock64() - mv0));
#endif
                float e[N];
                check_end_round<N>(s, r, e);
#pragma unroll
                for (int i = 0; i < N; i++) {
                    ended |= e[i] != 0.f;
                    ended_out[(ob + b) * N + i] = e[i];
                }
                RT_MARK(7)
                action_out[ob + b] = (int16_t)a;
                if (ended) {
                    nxt = 0;
                    gdone[b] += 1;
                }
                pl[b] = (int8_t)nxt;
            }
            RT_MARK(2)
#if ROLLOUT_TIMING
            {   // per wave: move pipeline up to the deals (24+w)
                if (l == 0) atomicAdd((unsigned long long *)&spl_probe_acc[24 + w], (unsigned long long)(clock64() - mv0));
            }
#endif
            for (uint64_t rm = __ballot(ended); rm; rm &= rm - 1) {
                const int rb = __shfl(b, __ffsll((unsigned long long)rm) - 1);
                const int g = gdone[rb];                      // the new game's number
                const int slot = g - gd0[rb] - 1;
                if (slot < pre) {
                    wave_apply_deal<N>(lds + rb * ST, drec[slot][rb], tabs.view());
                    RT_MARK(8)
                } else {
                    wave_philox_uniforms(ub[w], seed, bbase + (uint32_t)(b0 + rb), DEAL_STREAM | (uint32_t)g, 0,
                                         DEAL_DRAWS);
                    RT_MARK(9)
                    wave_init_game<N>(lds + rb * ST, ub[w], tabs.view());
                    RT_MARK(8)
                }
            }
#if ROLLOUT_TIMING
            if (l == 0) atomicAdd((unsigned long long *)&spl_probe_acc[20 + w], (unsigned long long)(clock64() - mv0));
#endif
            if (ROLLOUT_PRIO) __builtin_amdgcn_s_setprio(0);
        }
        lds_sync();
        RT_MARK(3)
    }
    for (int i = tid; i < nb * Cv::UNITS; i += THREADS) {
        const int b = i / Cv::UNITS, u = i - b * Cv::UNITS;
        Cv::store(gst + (size_t)b * Lx::S, lds + b * ST, u);
    }
    if (tid < nb) {
        player[b0 + tid] = pl[tid];
        if (games_done) games_done[b0 + tid] = gdone[tid];
    }
#if ROLLOUT_TIMING
    __syncthreads();
    RT_MARK(4)
    if (threadIdx.x == 0) {
        uint64_t *o = g_rollout_timing + (size_t)blockIdx.x * 40;   // tools/time_rollout.hip row
        for (int k = 0; k < 24; k++) o[k] = spl_probe_acc[k];
        o[24] = wall0;
        o[25] = wall_clock64();
        for (int k = 24; k < 32; k++) o[k + 2] = spl_probe_acc[k];   // o[26..29] pre-deal, o[30..33] make_move done
    }
#endif
}

// Board.get_symmetries (SplendorLogicNumba.py:349-395) for E examples, one wave per
// example. Variant k of K = 10 + 2n: 0 = identity; 1..9 = tier t = (k-1)/3 visible cards
// permuted by cards_symmetries[(k-1)%3] (SplendorLogic.py:283) with buy/reserve actions
// permuted alike; 10 + 2p + q = player p's reserved cards permuted by
// reserve_symmetries[#reserved][q] (:284-295; present only when defined), buy-reserve
// actions permuted for p == 0. present[e][k] marks emitted variants (reference order).
__constant__ int8_t K_CARD_SYM[3][4] = {{1, 3, 0, 2}, {2, 0, 3, 1}, {3, 2, 1, 0}};
__constant__ int8_t K_RSV_SYM[4][2][3] = {{{-1, -1, -1}, {-1, -1, -1}}, {{-1, -1, -1}, {-1, -1, -1}},
                                          {{1, 0, 2}, {-1, -1, -1}}, {{1, 2, 0}, {2, 0, 1}}};

// _nb_of_reserved_cards (:770-774) of player p: the first empty reserve slot
template <int N>
__device__ __forceinline__ int nb_reserved(const int8_t *s, int p) {
    int r = 3;
    for (int c = 2; c >= 0; c--)
        if (sum5(HbmRows{s}(Lay<N>::RSV + 6 * p + 2 * c)) == 0) r = c;
    return r;
}
// Source of state byte i / action a in the variant that permutes tier `tier`'s visible cards
// (tier >= 0) or player p's reserved cards (p >= 0) by perm; identity: tier = p = -1.
template <int N>
__device__ __forceinline__ int sym_src_byte(int i, int tier, int p, const int8_t *perm) {
    using Lx = Lay<N>;
    const int r = i / 7, c = i - 7 * (i / 7);
    if (tier >= 0 && r >= Lx::TIERS + 8 * tier && r < Lx::TIERS + 8 * tier + 8) {
        const int rr = r - Lx::TIERS - 8 * tier;
        return 7 * (Lx::TIERS + 8 * tier + 2 * perm[rr >> 1] + (rr & 1)) + c;
    }
    if (p >= 0 && r >= Lx::RSV + 6 * p && r < Lx::RSV + 6 * p + 6) {
        const int rr = r - Lx::RSV - 6 * p;
        return 7 * (Lx::RSV + 6 * p + 2 * perm[rr >> 1] + (rr & 1)) + c;
    }
    return i;
}
__device__ __forceinline__ int sym_src_action(int a, int tier, int p, const int8_t *perm) {
    int src = a;
    if (tier >= 0) {
        if (a >= 4 * tier && a < 4 * tier + 4) src = 4 * tier + perm[a - 4 * tier];
        if (a >= 12 + 4 * tier && a < 16 + 4 * tier) src = 12 + 4 * tier + perm[a - 12 - 4 * tier];
    }
    if (p == 0 && a >= 27 && a < 30) src = 27 + perm[a - 27];
    return src;
}

template <int N>
__global__ __launch_bounds__(THREADS) void k_symmetries(int E, const int8_t *__restrict__ state,
                                                        const float *__restrict__ pi,
                                                        const uint64_t *__restrict__ valid,
                                                        int8_t *__restrict__ ostate, float *__restrict__ opi,
                                                        uint64_t *__restrict__ ovalid,
                                                        uint8_t *__restrict__ present) {
    using Lx = Lay<N>;
    constexpr int K = 10 + 2 * N;
    __shared__ __align__(16) int8_t lds[WAVES][(Lx::S + 15) & ~15];   // raw 7-byte rows
    const int w = threadIdx.x >> 6, e = blockIdx.x * WAVES + w;
    if (e >= E) return;
    const int l = lane_id();
    int8_t *s = lds[w];
    wave_copy_bytes(s, state + (size_t)e * Lx::S, Lx::S);
    int nres[N];
#pragma unroll
    for (int p = 0; p < N; p++) nres[p] = nb_reserved<N>(s, p);
    for (int k = 0; k < K; k++) {
        int tier = -1, p = -1;
        const int8_t *perm = nullptr;
        if (k >= 1 && k <= 9) { tier = (k - 1) / 3; perm = K_CARD_SYM[(k - 1) % 3]; }
        if (k >= 10) {
            p = (k - 10) / 2;
            perm = K_RSV_SYM[nres[p]][(k - 10) % 2];
            if (perm[0] < 0) { if (l == 0) present[(size_t)e * K + k] = 0; continue; }
        }
        if (l == 0) present[(size_t)e * K + k] = 1;
        int8_t *os = ostate + ((size_t)e * K + k) * Lx::S;
        // state bytes: rows of the permuted block come from the source row pair
        for (int i = l; i < Lx::S; i += 64) os[i] = s[sym_src_byte<N>(i, tier, p, perm)];
        // policy and legality: action a takes the source action's entry
        const float *ip = pi + (size_t)e * SPL_ACTIONS;
        float *op = opi + ((size_t)e * K + k) * SPL_ACTIONS;
        const uint64_t *iv = valid + (size_t)e * 7;
#pragma unroll
        for (int ch = 0; ch < 7; ch++) {
            const int a = 64 * ch + l;
            const int src = sym_src_action(a, tier, p, perm);
            if (a < SPL_ACTIONS) op[a] = ip[src];
            const bool bit = a < SPL_ACTIONS && ((iv[src >> 6] >> (src & 63)) & 1);
            const uint64_t word = __ballot(bit);
            if (l == 0) ovalid[((size_t)e * K + k) * 7 + ch] = word;
        }
    }
}

// Variants Board.get_symmetries emits for a board: 10 + sum over players of
// (0, 0, 1, 2)[#reserved]. ~30 bytes read per board: one lane per board straight from HBM.
template <int N>
__global__ __launch_bounds__(256) void k_symmetry_counts(int E, const int8_t *__restrict__ state,
                                                         uint8_t *__restrict__ count) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int8_t *s = state + (size_t)e * Lay<N>::S;
    int k = 10;
#pragma unroll
    for (int p = 0; p < N; p++) {
        const int nr = nb_reserved<N>(s, p);
        k += nr >= 2 ? nr - 1 : 0;
    }
    count[e] = (uint8_t)k;
}

// Training rows from unexpanded examples, one wave per output row: row i is variant number
// ordinal[i] (among the variants k_symmetries marks present, in its order) of example
// example[i], written as the network's input (board cast to f32), the permuted policy, the
// permuted legality as one byte per action, and the example's winner / scdiff. The source
// board is staged in the wave's LDS slot; #reserved is read only for the players the
// ordinal walks over. A row whose example or ordinal is out of range reads nothing, is
// written as zeros and ORs SPL_ERR_BAD_INDEX into *err.
template <int N>
__global__ __launch_bounds__(THREADS) void k_gather_examples(
    int E, int M, const int8_t *__restrict__ state, const float *__restrict__ pi,
    const uint64_t *__restrict__ valid, const float *__restrict__ winner,
    const int32_t *__restrict__ scdiff, const int64_t *__restrict__ example,
    const int32_t *__restrict__ ordinal, float *__restrict__ x, float *__restrict__ opi,
    uint8_t *__restrict__ ovalid, float *__restrict__ owinner, int32_t *__restrict__ oscdiff,
    int32_t *err) {
    using Lx = Lay<N>;
    __shared__ __align__(16) int8_t lds[WAVES][(Lx::S + 15) & ~15];   // raw 7-byte rows
    const int w = threadIdx.x >> 6, i = blockIdx.x * WAVES + w;
    if (i >= M) return;
    const int l = lane_id();
    const int64_t e = (int64_t)uniform64((uint64_t)example[i]);
    const int k = uniform(ordinal[i]);
    int8_t *s = lds[w];
    float *ox = x + (size_t)i * Lx::S;
    float *op = opi + (size_t)i * SPL_ACTIONS;
    uint8_t *ov = ovalid + (size_t)i * SPL_ACTIONS;
    // dword stores of the 409 legality bytes: `head` bytes up to the first aligned address,
    // nd dwords, then the tail (rows are 409 bytes, so the alignment differs row to row)
    const int head = (int)((4 - ((uintptr_t)ov & 3)) & 3);
    const int nd = (SPL_ACTIONS - head) >> 2, tail = head + 4 * nd;

    bool ok = e >= 0 && e < E && k >= 0;
    int tier = -1, p = -1;
    const int8_t *perm = K_CARD_SYM[0];
    if (ok) {
        wave_copy_bytes(s, state + (size_t)e * Lx::S, Lx::S);
        __builtin_amdgcn_wave_barrier();
        if (k >= 1 && k <= 9) {
            tier = (k - 1) / 3;
            perm = K_CARD_SYM[(k - 1) % 3];
        } else if (k >= 10) {            // the (k-10)-th defined reserve permutation, players in order
            int rem = k - 10;
            ok = false;
            for (int q = 0; q < N && !ok; q++) {
                const int nr = uniform(nb_reserved<N>(s, q));
                const int c = nr >= 2 ? nr - 1 : 0;
                if (rem < c) {
                    p = q;
                    perm = K_RSV_SYM[nr][rem];
                    ok = true;
                }
                rem -= c;
            }
        }
    }
    if (!ok) {
        for (int j = l; j < Lx::S; j += 64) ox[j] = 0.f;
        for (int a = l; a < SPL_ACTIONS; a += 64) op[a] = 0.f;
        if (l < head) ov[l] = 0;
        for (int d = l; d < nd; d += 64) *reinterpret_cast<uint32_t *>(ov + head + 4 * d) = 0u;
        if (tail + l < SPL_ACTIONS) ov[tail + l] = 0;
        if (l < N) {
            owinner[(size_t)i * N + l] = 0.f;
            oscdiff[(size_t)i * N + l] = 0;
        }
        if (err && l == 0) atomicOr(err, SPL_ERR_BAD_INDEX);
        return;
    }
    for (int j = l; j < Lx::S; j += 64) ox[j] = (float)s[sym_src_byte<N>(j, tier, p, perm)];
    const float *ip = pi + (size_t)e * SPL_ACTIONS;
    for (int a = l; a < SPL_ACTIONS; a += 64) op[a] = ip[sym_src_action(a, tier, p, perm)];
    // the 7 mask words are wave-uniform (scalar loads); a lane picks its word by selects, so
    // they stay in registers (an indexed array would be spilled to LDS or scratch)
    const uint64_t *iv = valid + (size_t)e * SPL_MASK_WORDS;
    const uint64_t v0 = iv[0], v1 = iv[1], v2 = iv[2], v3 = iv[3], v4 = iv[4], v5 = iv[5], v6 = iv[6];
    auto legal = [=](int a) -> uint32_t {
        const int src = sym_src_action(a, tier, p, perm), c = src >> 6;
        const uint64_t word = c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : c == 3 ? v3 : c == 4 ? v4 : c == 5 ? v5 : v6;
        return (uint32_t)(word >> (src & 63)) & 1u;
    };
    if (l < head) ov[l] = (uint8_t)legal(l);
    for (int d = l; d < nd; d += 64) {
        const int a = head + 4 * d;
        *reinterpret_cast<uint32_t *>(ov + a) =
            legal(a) | legal(a + 1) << 8 | legal(a + 2) << 16 | legal(a + 3) << 24;
    }
    if (tail + l < SPL_ACTIONS) ov[tail + l] = (uint8_t)legal(tail + l);
    if (l < N) {
        owinner[(size_t)i * N + l] = winner[(size_t)e * N + l];
        oscdiff[(size_t)i * N + l] = scdiff[(size_t)e * N + l];
    }
}

// ---------------------------------------------------------------- launch helpers
inline int check_launch() { return hipGetLastError() == hipSuccess ? 0 : SPL_EDEVICE; }
inline dim3 wave_grid(int B) { return dim3((unsigned)((B + WAVES - 1) / WAVES)); }
inline dim3 lane_grid(int B) { return dim3((unsigned)((B + 255) / 256)); }
// the `lim` argument of the mask-building kernels: token limit and rules (splendor_device.h)
inline int ctx_lim(const spl_ctx *c) { return pack_lim(c->token_limit, c->rules); }

#define SPL_DISPATCH(n, CALL)            \
    switch (n) {                         \
        case 2: { constexpr int N = 2; CALL; break; } \
        case 3: { constexpr int N = 3; CALL; break; } \
        default: { constexpr int N = 4; CALL; break; } \
    }

}  // namespace

// ---------------------------------------------------------------- C ABI
extern "C" {

int spl_abi_version(void) { return SPL_ABI_VERSION; }

int spl_ctx_create(int n, int token_limit, spl_ctx **out) {
    if (!out || n < 2 || n > 4 || token_limit < 3 || token_limit > 100) return SPL_EINVAL;
    spl_ctx *c = new (std::nothrow) spl_ctx;
    if (!c) return SPL_EINVAL;
    c->n = n;
    c->token_limit = token_limit;
    c->rules = 0;
    *out = c;
    return 0;
}

int spl_ctx_destroy(spl_ctx *ctx) {
    delete ctx;
    return 0;
}

int spl_state_rows(const spl_ctx *c) { return ok_ctx(c) ? 32 + 10 * c->n + c->n * c->n : SPL_EINVAL; }
int spl_state_bytes(const spl_ctx *c) { return ok_ctx(c) ? 7 * spl_state_rows(c) : SPL_EINVAL; }

int spl_init(const spl_ctx *c, int B, int8_t *state, int8_t *player_out, const double *u,
             int u_stride, uint64_t seed, uint32_t stream, uint32_t board_base, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && !state) || (u && u_stride < 29)) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_init<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, state, player_out, u, u_stride,
                                          seed, stream, board_base));
    return check_launch();
}

int spl_valid_moves(const spl_ctx *c, int B, const int8_t *state, const int8_t *player,
                    uint64_t *mask, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !mask))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_valid<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, state, player, ctx_lim(c), mask));
    return check_launch();
}

int spl_step(const spl_ctx *c, int B, int8_t *state, const int8_t *player, const int16_t *action,
             int8_t *next_player, int det, const double *u, int u_stride, uint64_t seed,
             uint32_t stream, uint32_t board_base, int32_t *err, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !action)) || (u && u_stride < 2)) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_step<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, state, player, action, next_player,
                                          det, u, u_stride, seed, stream, board_base, err));
    return check_launch();
}

int spl_game_ended(const spl_ctx *c, int B, const int8_t *state, float *out, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !out))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_ended<N>, lane_grid(B), dim3(256), 0,
                                          (hipStream_t)hs, B, state, out));
    return check_launch();
}

int spl_canonical(const spl_ctx *c, int B, const int8_t *state, const int8_t *player,
                  int8_t *out, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !out))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_canonical<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, state, player, out));
    return check_launch();
}

int spl_score(const spl_ctx *c, int B, const int8_t *state, int32_t *out, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !out))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_score_round<N>, lane_grid(B), dim3(256), 0,
                                          (hipStream_t)hs, B, state, out, (int32_t *)nullptr));
    return check_launch();
}

int spl_round(const spl_ctx *c, int B, const int8_t *state, int32_t *out, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!state || !out))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_score_round<N>, lane_grid(B), dim3(256), 0,
                                          (hipStream_t)hs, B, state, (int32_t *)nullptr, out));
    return check_launch();
}

int spl_tree_step(const spl_ctx *c, int B, const int8_t *parent, const int16_t *action,
                  int8_t *child, int32_t *err, void *hs) {
    if (!ok_ctx(c) || B < 0 || (B && (!parent || !action || !child))) return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_tree_step<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, parent, action, child, err));
    return check_launch();
}

int spl_player_move(const spl_ctx *c, int B, const int8_t *state, const uint8_t *active, int kind,
                    const float *pi, uint64_t seed, uint32_t stream, uint32_t board_base,
                    int16_t *action, uint64_t *cand_out, int32_t *best_out, void *hs) {
    if (!ok_ctx(c) || !state || !action || B < 0 || kind < SPL_PLAYER_RANDOM || kind > SPL_PLAYER_POLICY ||
        (kind == SPL_PLAYER_POLICY && !pi) || stream > 0xFFFFFFu)
        return SPL_EINVAL;
    if (!B) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_player_move<N>, wave_grid(B), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, state, active, kind, pi, ctx_lim(c),
                                          seed, stream, board_base, action, cand_out, best_out));
    return check_launch();
}

int spl_ctx_set_token_limit(spl_ctx *c, int token_limit) {
    if (!ok_ctx(c) || token_limit < 3 || token_limit > 100) return SPL_EINVAL;
    c->token_limit = token_limit;
    return 0;
}

int spl_ctx_set_rules(spl_ctx *c, int flags) {
    if (!ok_ctx(c) || (flags & ~SPL_RULE_NO_RESERVE)) return SPL_EINVAL;
    c->rules = flags;
    return 0;
}

int spl_ctx_rules(const spl_ctx *c) { return ok_ctx(c) ? c->rules : SPL_EINVAL; }

int spl_symmetries(const spl_ctx *c, int E, const int8_t *state, const float *pi,
                   const uint64_t *valid, int8_t *out_state, float *out_pi, uint64_t *out_valid,
                   uint8_t *present, void *hs) {
    if (!ok_ctx(c) || E < 0 || (E && (!state || !pi || !valid || !out_state || !out_pi || !out_valid ||
                                      !present)))
        return SPL_EINVAL;
    if (!E) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_symmetries<N>, wave_grid(E), dim3(THREADS), 0,
                                          (hipStream_t)hs, E, state, pi, valid, out_state, out_pi,
                                          out_valid, present));
    return check_launch();
}

int spl_symmetry_counts(const spl_ctx *c, int E, const int8_t *state, uint8_t *count, void *hs) {
    if (!ok_ctx(c) || E < 0 || (E && (!state || !count))) return SPL_EINVAL;
    if (!E) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_symmetry_counts<N>, lane_grid(E), dim3(256), 0,
                                          (hipStream_t)hs, E, state, count));
    return check_launch();
}

int spl_gather_examples(const spl_ctx *c, int E, int M, const int8_t *state, const float *pi,
                        const uint64_t *valid, const float *winner, const int32_t *scdiff,
                        const int64_t *example, const int32_t *ordinal, float *x, float *out_pi,
                        uint8_t *out_valid, float *out_winner, int32_t *out_scdiff, int32_t *err,
                        void *hs) {
    if (!ok_ctx(c) || E < 0 || M < 0 ||
        (E && M && (!state || !pi || !valid || !winner || !scdiff || !example || !ordinal || !x ||
                    !out_pi || !out_valid || !out_winner || !out_scdiff)))
        return SPL_EINVAL;
    if (!E || !M) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_gather_examples<N>, wave_grid(M), dim3(THREADS), 0,
                                          (hipStream_t)hs, E, M, state, pi, valid, winner, scdiff,
                                          example, ordinal, x, out_pi, out_valid, out_winner,
                                          out_scdiff, err));
    return check_launch();
}

int spl_rollout_run(const spl_ctx *c, int B, int K, int8_t *state, int8_t *player, uint64_t *mask_out,
                    int16_t *action_out, float *ended_out, int32_t *games_done, uint64_t seed,
                    uint32_t step0, uint32_t board_base, void *hs) {
    if (!ok_ctx(c) || B < 0 || K < 0 || (B && K && (!state || !player || !action_out || !ended_out || !games_done)))
        return SPL_EINVAL;
    if (!B || !K) return 0;
    SPL_DISPATCH(c->n, hipLaunchKernelGGL(k_rollout<N>, dim3((unsigned)((B + RB - 1) / RB)), dim3(THREADS), 0,
                                          (hipStream_t)hs, B, K, state, player, ctx_lim(c),
                                          mask_out, action_out, ended_out, games_done, seed,
                                          step0, board_base));
    return check_launch();
}

int spl_rollout_step(const spl_ctx *c, int B, int8_t *state, int8_t *player, uint64_t *mask_out,
                     int16_t *action_out, float *ended_out, int32_t *games_done, uint64_t seed,
                     uint32_t step, uint32_t board_base, void *hs) {
    if (B && !mask_out) return SPL_EINVAL;
    return spl_rollout_run(c, B, 1, state, player, mask_out, action_out, ended_out, games_done, seed,
                           step, board_base, hs);
}

}  // extern "C"
