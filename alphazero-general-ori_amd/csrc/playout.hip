// playout.hip — spl_playout (include/splendor_amd.h): random playouts of a batch of positions
// to the end of the game, only the outcomes leave the chip. The leaf evaluation of the
// network-free search players (splendor/playout.py) and Monte-Carlo outcome estimates.
//
// A step is k_rollout's (splendor_env.hip) without the re-deal and without per-move outputs:
// both kernels call the same phases (board_phases.h: table staging, predicates, mask words,
// quad select, move by wave kind), so a uniform playout repeats the rollout's moves bit for
// bit. What is this kernel's own: the live / active flags, the buy-first filter, the uniform
// prior and the outcome sums. Mapping: a 256-thread workgroup owns 64 / P consecutive rows
// and their (64 / P) P <= 64 tasks (task l = playout l % P of row r0 + l / P), a lane per
// task, each task's board in its own LDS slot (8-byte rows, odd qword stride) for the whole
// playout. A row's P tasks therefore always share a workgroup: the row's result is summed in
// LDS in task order at the end of the launch, with no scratch memory, second launch or
// floating-point atomic (P = 1, 2, 4, .., 64 fill every lane; other P leave 64 % P idle).
// The move loop is bounded by max_steps and touches no HBM; a task that has ended (or whose
// row is inactive) is predicated off, every wave reaches every barrier, and the workgroup
// leaves the loop when none of its tasks is live.
//
// spl_playout_seq runs the same kernel with the stream base read from a device counter (SEQ:
// step0 = (*call_seq mod 2^23) 256, so a captured launch draws new streams at every replay)
// and, given the search's NN-leaf list (LIST), on the listed rows only: a workgroup then owns
// 64 / P consecutive list entries, found by the network kernel's scan of the segment counts
// (nn_stage.h leaf_list_scan), and one past the
// end of the list leaves before it stages anything. Task keys stay tied to the row.
//
// spl_playout_mix (MIX, with SEQ) blends instead of storing: v = (1 - lambda) v + lambda mean in
// the caller's value buffer (the network's), lambda one device f32 clamped to 0..1; the priors
// stay the caller's, so no pi_out and no steps_out. A clamped lambda of 0 ends every workgroup
// before it stages anything.
#include <hip/hip_runtime.h>

#include "../../include/splendor_amd.h"
#include "board_phases.h"
#include "nn_stage.h"   // leaf_list_scan
#include "spl_ctx.h"

using namespace spl;

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int PT = 64;                           // task slots per workgroup (lane per task)
constexpr uint64_t BUY_BITS = 0x38000FFFull;     // actions 0-11 (buy visible), 27-29 (buy reserved)

// SEQ: the stream base is (*call_seq mod 2^23) SPL_PLAYOUT_SEQ_STREAMS instead of step0 (spl_playout_seq).
// LIST (with SEQ): the rows are the entries of the leaf list; r0 / nr / nb then count list entries
// and erow[] holds each entry's row (-1: an index outside 0 .. B - 1, which runs nothing).
// MIX (with SEQ): result is read and written, result = (1 - *lambda) result + *lambda mean, by the
// thread that stores the mean otherwise; pi_out and steps_out are not written.
template <int N, bool SEQ, bool LIST, bool MIX = false>
__global__ __launch_bounds__(THREADS) void k_playout(int B, int P, const int8_t *__restrict__ state,
                                                     const int8_t *__restrict__ player,
                                                     const uint8_t *__restrict__ active, int lim, int policy,
                                                     int max_steps, uint64_t seed, uint32_t step0, uint32_t bbase,
                                                     float *__restrict__ result, float *__restrict__ pi_out,
                                                     int32_t *__restrict__ steps_out, int32_t *unfinished,
                                                     const int32_t *__restrict__ leaf_index,
                                                     const int32_t *__restrict__ leaf_count,
                                                     const uint32_t *__restrict__ call_seq,
                                                     const float *__restrict__ lambda) {
    static_assert(SEQ || !LIST, "the list entry reads its stream base on the device");
    static_assert(SEQ || !MIX, "the mixed entry reads its stream base on the device");
    // one scalar for the whole grid: a block-uniform exit with no barrier before it (a NaN
    // clamps to 0: fmaxf returns its other operand)
    float lam = 0.f;
    if constexpr (MIX) {
        lam = fminf(fmaxf(*lambda, 0.f), 1.f);
        if (lam == 0.f) return;
    }
    using Lx = Lay<N>;
    using Cv = Conv<N>;
    constexpr int ST = RolloutLds<N>::STRIDE;
    constexpr int PER = PT / WAVES;
    static_assert(PER * 4 == 64, "select: four lanes per task, one wave per PER tasks");
    __shared__ __align__(16) int8_t lds[PT * ST];
    __shared__ uint64_t msk[PT][7];    // legality masks (odd qword stride: conflict-free)
    __shared__ int8_t pl[PT];          // player to move
    __shared__ uint8_t act[PT];        // the task's row is active (it runs and writes outputs)
    __shared__ uint8_t live[PT];       // the task is still playing
    __shared__ float outc[PT][N];      // outcome (zero until the game ends)
    __shared__ int32_t nstep[PT];      // moves played (max_steps until the game ends)
    __shared__ double ud[PT][4];       // draws 0..3 of each task's step stream
    __shared__ TabsLds tabs;
    __shared__ uint64_t mfac[MASK_FACTOR_WORDS];
    __shared__ uint32_t klist[4][PT];  // per move kind (file_move)
    __shared__ int kcount[4];
    __shared__ PredLds<PT> pred;
    __shared__ int erow[LIST ? PT : 1], eoff[LIST ? PT : 1];
    const int rpw = PT / P;                                  // rows (LIST: list entries) per workgroup
    // the wave index in an SGPR: the per-wave choices of the shared phases (board_phases.h) are
    // scalar branches. (k_rollout says why.)
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = lane_id();
    const int r0 = blockIdx.x * rpw;
    int nr = min(rpw, B - r0), lpos = 0;
    if constexpr (LIST) {
        // every wave scans the counts in registers, so the exit is block-uniform with no barrier
        // before it; wave 0 also resolves the workgroup's entries (plain 4-byte count loads: the
        // counts need no alignment here)
        const int total = nnstage::leaf_list_scan<PT, 4, false>(leaf_count, (B + 63) >> 6, r0, w == 0 ? erow : nullptr,
                                                                w == 0 ? eoff : nullptr, lpos);
        if (r0 >= total) return;
        nr = min(rpw, total - r0);
    }
    const int nb = nr * P;
    const int lrow = l / P;                                  // task l = playout l - lrow * P of row r0 + lrow
    uint32_t board = bbase + (uint32_t)(r0 + lrow) * (uint32_t)P + (uint32_t)(l - lrow * P);
    if constexpr (SEQ) step0 = (*call_seq & 0x7FFFFFu) * (uint32_t)SPL_PLAYOUT_SEQ_STREAMS;
    // prologue: the table loads go out first, the boards load while they are in flight
    {
        TabsRegs<THREADS> q_tabs;
        q_tabs.fetch(tid);
        if constexpr (LIST) {
            __builtin_amdgcn_wave_barrier();                 // (wave 0 has read its eoff[] above)
            if (w == 0) {
                int r = -1;
                if (l < nr && lpos < B) r = leaf_index[lpos];
                erow[l] = r >= 0 && r < B ? r : -1;
            }
            lds_sync();
        }
        if (tid < PT) {
            const bool on = tid < nb && (LIST ? erow[lrow] >= 0 : !active || active[r0 + lrow]);
            act[tid] = on;
            live[tid] = on;
            pl[tid] = !LIST && on && player ? player[r0 + lrow] : (int8_t)0;
            nstep[tid] = max_steps;
#pragma unroll
            for (int i = 0; i < N; i++) outc[tid][i] = 0.f;
        }
        // every task gets its own copy of its row's board (the P reads of a row hit the cache)
        for (int i = tid; i < nb * Cv::UNITS; i += THREADS) {
            const int t = i / Cv::UNITS, u = i - t * Cv::UNITS, r = LIST ? erow[t / P] : r0 + t / P;
            if (LIST ? r >= 0 : !active || active[r]) Cv::load(lds + t * ST, state + (size_t)r * Lx::S, u);
        }
        if (tid < 4) kcount[tid] = 0;
        q_tabs.put(tabs, mfac, tid);
    }
    lds_sync();
    const int myrow = LIST ? erow[lrow] : r0 + lrow;         // (the key stays the row's, not the entry's)
    if constexpr (LIST) board = bbase + (uint32_t)myrow * (uint32_t)P + (uint32_t)(l - lrow * P);
    for (int t = 0; t < max_steps; ++t) {
        const uint32_t step = step0 + (uint32_t)t;
        if (tid < 4) kcount[tid] = 0;                    // (last read in the previous move phase)
        const bool on = l < nb && live[l];               // (live changes in the move phase only)
        // predicates: wave w computes part w of every live task's predicate set (lane per task);
        // wave 3 (the lightest part) also draws Philox blocks 0-1 of the task's step stream
        if (w == 2) __builtin_amdgcn_s_setprio(1);
        if (w == 3 && on) {
#pragma unroll
            for (int k = 0; k < 2; k++) philox_pair(seed, board, step, k, ud[l][2 * k], ud[l][2 * k + 1]);
        }
        if (on) phase_predicates<N>(w, l, lds + l * ST, pl[l], lim, pred);
        __builtin_amdgcn_s_setprio(0);
        lds_sync();
        // mask words w and w+4 of every live task
        if (on) phase_mask_words<N>(w, l, lds + l * ST, pl[l], lim, pred, mfac, msk[l]);
        lds_sync();
        // the uniform prior over the input board's legal moves: once per active row, from the
        // first mask of its task 0 (pass alone when nothing else is legal). Block-uniform.
        if (!MIX && t == 0 && pi_out) {
            for (int b = 0; b < nb; b += P) {
                if (!act[b]) continue;
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < 7; k++) cnt += __popcll(msk[b][k]);
                const float inv = 1.0f / (float)max(cnt, 1);
                float *po = pi_out + (size_t)(LIST ? erow[b / P] : r0 + b / P) * SPL_ACTIONS;
                for (int a = tid; a < SPL_ACTIONS; a += THREADS) {
                    const bool bit = cnt ? (msk[b][a >> 6] >> (a & 63)) & 1 : a == SPL_ACTIONS - 1;
                    po[a] = bit ? inv : 0.f;
                }
            }
        }
        // select: four lanes per task (task w*16 + l/4; lane q = l%4 holds mask words 2q, 2q+1),
        // quad_select. BUY_FIRST keeps only the buy bits of word 0 when there are any. Pass when
        // nothing is legal; the task is filed by move kind.
        {
            const int b = w * PER + (l >> 2), q = l & 3;
            const bool sel = b < nb && live[b];
            uint64_t x0 = 0, x1 = 0;
            if (sel) {
                x0 = msk[b][2 * q];
                if (q < 3) x1 = msk[b][2 * q + 1];
            }
            const int buys = quad_bcast<0>((int)(policy == SPL_PLAYOUT_BUY_FIRST && (x0 & BUY_BITS) != 0));
            if (buys) {
                x0 = q == 0 ? x0 & BUY_BITS : 0;
                x1 = 0;
            }
            const QuadPick pk = quad_select(x0, x1, q, sel ? ud[b][0] : 0.0);
            const int a = sel && pk.cnt == 0 && q == 3 ? SPL_ACTIONS - 1 : pk.a;
            if (a >= 0) file_move(klist, kcount, b, a, pl[b]);
        }
        lds_sync();
        // move: wave k makes the moves of kind k, lane per task: chance draws 1-2, end check
        {
            const int kc = kcount[w];
            const uint32_t ke = klist[w][l];                 // (read before the count is known)
            if (w == MK_BUY || w == MK_RESERVE) __builtin_amdgcn_s_setprio(2);
            if (l < kc) {
                const int b = ke & 0xFF, a = (ke >> 8) & 0xFFF, p = ke >> 20;
                int8_t *s = lds + b * ST;
                int r;                                            // the round after the move
                const int nxt = lane_move_of_kind<N>(w, s, a, p, &ud[b][0], tabs.view(), r);
                float e[N];
                check_end_round<N>(s, r, e);
                bool ended = false;
#pragma unroll
                for (int i = 0; i < N; i++) ended |= e[i] != 0.f;
                if (ended) {
#pragma unroll
                    for (int i = 0; i < N; i++) outc[b][i] = e[i];
                    nstep[b] = t + 1;
                    live[b] = 0;
                }
                pl[b] = (int8_t)nxt;
            }
            __builtin_amdgcn_s_setprio(0);
        }
        lds_sync();
        // every wave reads the same 64 flags after the barrier: a block-uniform exit
        if (__ballot(l < nb && live[l]) == 0) break;
    }
    // outputs, once: a row's mean is the f32 sum of its P outcomes in task order, over (float)P
    if (tid < nr * N) {
        const int rr = tid / N, i = tid - rr * N;
        if (act[rr * P]) {
            float sum = 0.f;
            for (int j = 0; j < P; j++) sum += outc[rr * P + j][i];
            if constexpr (MIX) {
                float *out = result + (size_t)(LIST ? erow[rr] : r0 + rr) * N + i;
                *out = (1.0f - lam) * *out + lam * (sum / (float)P);
            } else {
                result[(size_t)(LIST ? erow[rr] : r0 + rr) * N + i] = sum / (float)P;
            }
        }
    }
    if (w == 0) {
        const bool on = l < nb && act[l];
        if (!MIX && steps_out && on)
            steps_out[LIST ? (size_t)myrow * P + (l - lrow * P) : (size_t)r0 * P + l] = nstep[l];
        const uint64_t open = __ballot(l < nb && live[l]);   // still playing after max_steps moves
        if (unfinished && open && l == 0) atomicAdd(unfinished, (int32_t)__popcll(open));
    }
}

// one launch of k_playout<N, SEQ, LIST, MIX>; a list launch is sized for B entries (the host cannot
// know the list's length: the workgroups past its end leave at once)
template <bool SEQ, bool LIST, bool MIX = false>
int launch_playout(const spl_ctx *c, int B, const int8_t *state, const int8_t *player, const uint8_t *active,
                   int policy, int playouts, int max_steps, uint64_t seed, uint32_t step0, uint32_t board_base,
                   float *result, float *pi_out, int32_t *steps_out, int32_t *unfinished, const int32_t *leaf_index,
                   const int32_t *leaf_count, const uint32_t *call_seq, void *hs, const float *lambda = nullptr) {
    const int rpw = PT / playouts;
    const dim3 grid((unsigned)(((long long)B + rpw - 1) / rpw));
#define SPL_PLAYOUT_LAUNCH(NP)                                                                            \
    hipLaunchKernelGGL((k_playout<NP, SEQ, LIST, MIX>), grid, dim3(THREADS), 0, (hipStream_t)hs, B,      \
                       playouts, state, player, active, pack_lim(c->token_limit, c->rules), policy,       \
                       max_steps, seed, step0, board_base, result, pi_out, steps_out, unfinished,         \
                       leaf_index, leaf_count, call_seq, lambda)
    switch (c->n) {
        case 2: SPL_PLAYOUT_LAUNCH(2); break;
        case 3: SPL_PLAYOUT_LAUNCH(3); break;
        default: SPL_PLAYOUT_LAUNCH(4); break;
    }
#undef SPL_PLAYOUT_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : SPL_EDEVICE;
}

}  // namespace

extern "C" int spl_playout(const spl_ctx *c, int B, const int8_t *state, const int8_t *player,
                           const uint8_t *active, int policy, int playouts, int max_steps, uint64_t seed,
                           uint32_t step0, uint32_t board_base, float *result, float *pi_out,
                           int32_t *steps_out, int32_t *unfinished, void *hs) {
    if (!ok_ctx(c) || !state || !result || B < 0 || policy < SPL_PLAYOUT_UNIFORM ||
        policy > SPL_PLAYOUT_BUY_FIRST || playouts < 1 || playouts > 64 || max_steps < 1 || max_steps > 1024 ||
        (uint64_t)step0 + (uint64_t)max_steps > 0x80000000ull)
        return SPL_EINVAL;
    if (!B) return 0;
    return launch_playout<false, false>(c, B, state, player, active, policy, playouts, max_steps, seed, step0,
                                        board_base, result, pi_out, steps_out, unfinished, nullptr, nullptr, nullptr,
                                        hs);
}

extern "C" int spl_playout_seq(const spl_ctx *c, int B, const int8_t *state, const uint8_t *active,
                               const int32_t *leaf_index, const int32_t *leaf_count, int policy, int playouts,
                               int max_steps, uint64_t seed, const uint32_t *call_seq, uint32_t board_base,
                               float *result, float *pi_out, int32_t *steps_out, int32_t *unfinished, void *hs) {
    if (!ok_ctx(c) || !state || !result || !call_seq || B < 0 || policy < SPL_PLAYOUT_UNIFORM ||
        policy > SPL_PLAYOUT_BUY_FIRST || playouts < 1 || playouts > 64 || max_steps < 1 ||
        max_steps > SPL_PLAYOUT_SEQ_STREAMS || !leaf_index != !leaf_count || (active && leaf_index))
        return SPL_EINVAL;
    if (!B) return 0;
    if (leaf_index)
        return launch_playout<true, true>(c, B, state, nullptr, nullptr, policy, playouts, max_steps, seed, 0,
                                          board_base, result, pi_out, steps_out, unfinished, leaf_index, leaf_count,
                                          call_seq, hs);
    return launch_playout<true, false>(c, B, state, nullptr, active, policy, playouts, max_steps, seed, 0,
                                       board_base, result, pi_out, steps_out, unfinished, nullptr, nullptr, call_seq,
                                       hs);
}

extern "C" int spl_playout_mix(const spl_ctx *c, int B, const int8_t *state, const uint8_t *active,
                               const int32_t *leaf_index, const int32_t *leaf_count, int policy, int playouts,
                               int max_steps, uint64_t seed, const uint32_t *call_seq, uint32_t board_base,
                               const float *lambda, float *v, int32_t *unfinished, void *hs) {
    if (!ok_ctx(c) || !state || !v || !call_seq || !lambda || B < 0 || policy < SPL_PLAYOUT_UNIFORM ||
        policy > SPL_PLAYOUT_BUY_FIRST || playouts < 1 || playouts > 64 || max_steps < 1 ||
        max_steps > SPL_PLAYOUT_SEQ_STREAMS || !leaf_index != !leaf_count || (active && leaf_index))
        return SPL_EINVAL;
    if (!B) return 0;
    if (leaf_index)
        return launch_playout<true, true, true>(c, B, state, nullptr, nullptr, policy, playouts, max_steps, seed, 0,
                                                board_base, v, nullptr, nullptr, unfinished, leaf_index, leaf_count,
                                                call_seq, hs, lambda);
    return launch_playout<true, false, true>(c, B, state, nullptr, active, policy, playouts, max_steps, seed, 0,
                                             board_base, v, nullptr, nullptr, unfinished, nullptr, nullptr, call_seq,
                                             hs, lambda);
}
