// playout.hip — spl_playout (include/splendor_amd.h): random playouts of a batch of positions
// to the end of the game, only the outcomes leave the chip. The leaf evaluation of the
// network-free search players (splendor/playout.py) and Monte-Carlo outcome estimates.
//
// A step is k_rollout's (splendor_env.hip) without the re-deal and without per-move outputs,
// built from the same device functions (splendor_device.h), so a uniform playout repeats the
// rollout's moves bit for bit. Mapping: a 256-thread workgroup owns 64 / P consecutive rows
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
// 64 / P consecutive list entries, found by a scan of the segment counts, and one past the
// end of the list leaves before it stages anything. Task keys stay tied to the row.
#include <hip/hip_runtime.h>

#include "../../include/splendor_amd.h"
#include "splendor_device.h"

using namespace spl;

struct spl_ctx {  // must match splendor_env.hip
    int n;
    int token_limit;
    int rules;
};

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int PT = 64;                           // task slots per workgroup (lane per task)
constexpr uint64_t BUY_BITS = 0x38000FFFull;     // actions 0-11 (buy visible), 27-29 (buy reserved)

// COUNT elements of a constant table staged into LDS by the workgroup: every load is issued
// (clamped index, no branch) before the first LDS store, as k_rollout stages its tables
template <class T, int COUNT>
struct TableRegs {
    static constexpr int IT = (COUNT + THREADS - 1) / THREADS;
    T v[IT];
    __device__ __forceinline__ void fetch(const T *src, int tid) {
#pragma unroll
        for (int k = 0; k < IT; k++) v[k] = src[min(tid + k * THREADS, COUNT - 1)];
    }
    __device__ __forceinline__ void put(T *dst, int tid) const {
#pragma unroll
        for (int k = 0; k < IT; k++)
            if (tid + k * THREADS < COUNT) dst[tid + k * THREADS] = v[k];
    }
};

// The leaf list as spl_mcts_select_compact writes it: segment j (rows 64 j .. 64 j + 63) has
// count[j] entries at leaf_index[64 j ..]; the list is their concatenation in segment order.
// Wave-collective, registers only unless `slot` is given: returns the list's length, and with
// slot / offv (PT ints each, the calling wave's own) lane i gets the leaf_index position of list
// entry e0 + i in `pos` (meaningful for entries below the length). A lane holds 4 consecutive
// segments' counts and one DPP scan gives every segment's first entry, 256 segments per pass;
// each segment that reaches into [e0, e0 + PT) marks the slot where it starts (and 64 j - start
// in offv), and a prefix maximum over the slots gives every slot its segment (the scan of
// nn_list_rows, nnet.hip, on plain 4-byte loads: the counts need no alignment here).
__device__ __forceinline__ int list_rows(const int32_t *__restrict__ count, int nseg, int e0, int *slot, int *offv,
                                         int &pos) {
    const int lane = lane_id();
    if (slot) slot[lane] = -1;
    int base = 0;
    for (int c0 = 0; c0 < nseg; c0 += 4 * 64) {
        const int j0 = c0 + 4 * lane;
        int v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = min(max(count[min(j0 + q, nseg - 1)], 0), j0 + q < nseg ? 64 : 0);
        const int own = v[0] + v[1] + v[2] + v[3];
        // inclusive scan of the lanes' sums on DPP: row_shr 1 / 2 / 4 / 8 inside each 16-lane
        // row (lanes without a source add 0), then row_bcast 15 (rows 1, 3) and 31 (rows 2, 3)
        int inc = own;
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, true);
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xa, 0xf, false);
        inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xc, 0xf, false);
        if (slot) {
            int ex = base + inc - own;                   // first list entry of segment j0
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (v[q] > 0 && ex + v[q] > e0 && ex < e0 + PT) {
                    const int sl = max(ex - e0, 0);
                    slot[sl] = sl;
                    offv[sl] = 64 * (j0 + q) - ex;
                }
                ex += v[q];
            }
        }
        base += __builtin_amdgcn_readlane(inc, 63);
    }
    pos = 0;
    if (slot) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int f = slot[lane];                              // prefix maximum over slots 0 .. 63
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x111, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x112, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x114, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x118, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x142, 0xa, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x143, 0xc, 0xf, false));
        if (f >= 0) pos = e0 + lane + offv[f];
    }
    return base;
}

// SEQ: the stream base is (*call_seq mod 2^23) SPL_PLAYOUT_SEQ_STREAMS instead of step0 (spl_playout_seq).
// LIST (with SEQ): the rows are the entries of the leaf list; r0 / nr / nb then count list entries
// and erow[] holds each entry's row (-1: an index outside 0 .. B - 1, which runs nothing).
template <int N, bool SEQ, bool LIST>
__global__ __launch_bounds__(THREADS) void k_playout(int B, int P, const int8_t *__restrict__ state,
                                                     const int8_t *__restrict__ player,
                                                     const uint8_t *__restrict__ active, int lim, int policy,
                                                     int max_steps, uint64_t seed, uint32_t step0, uint32_t bbase,
                                                     float *__restrict__ result, float *__restrict__ pi_out,
                                                     int32_t *__restrict__ steps_out, int32_t *unfinished,
                                                     const int32_t *__restrict__ leaf_index,
                                                     const int32_t *__restrict__ leaf_count,
                                                     const uint32_t *__restrict__ call_seq) {
    static_assert(SEQ || !LIST, "the list entry reads its stream base on the device");
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
    __shared__ uint64_t mfac[7 * 116];  // K_MASK_FACTORS (lane_mask_word_fast)
    __shared__ uint32_t klist[4][PT];  // per move kind: task | action << 8 | player << 20
    __shared__ int kcount[4];
    __shared__ uint64_t pf0[WAVES][PT], pf1[PT];
    __shared__ uint32_t pcond[PT];
    __shared__ uint8_t pbad[WAVES][PT];
    __shared__ int erow[LIST ? PT : 1], eoff[LIST ? PT : 1];
    const int rpw = PT / P;                                  // rows (LIST: list entries) per workgroup
    const int tid = threadIdx.x, w = tid >> 6, l = lane_id();
    const int r0 = blockIdx.x * rpw;
    int nr = min(rpw, B - r0), lpos = 0;
    if constexpr (LIST) {
        // every wave scans the counts in registers, so the exit is block-uniform with no barrier
        // before it; wave 0 also resolves the workgroup's entries
        const int total = list_rows(leaf_count, (B + 63) >> 6, r0, w == 0 ? erow : nullptr, w == 0 ? eoff : nullptr,
                                    lpos);
        if (r0 >= total) return;
        nr = min(rpw, total - r0);
    }
    const int nb = nr * P;
    const int lrow = l / P;                                  // task l = playout l - lrow * P of row r0 + lrow
    uint32_t board = bbase + (uint32_t)(r0 + lrow) * (uint32_t)P + (uint32_t)(l - lrow * P);
    if constexpr (SEQ) step0 = (*call_seq & 0x7FFFFFu) * (uint32_t)SPL_PLAYOUT_SEQ_STREAMS;
    // prologue: the table loads go out first, the boards load while they are in flight
    {
        TableRegs<double, 41 * 9> q_quot;
        TableRegs<uint64_t, 240> q_cards;
        TableRegs<uint64_t, 409> q_take, q_give;
        TableRegs<int8_t, 409> q_rsv;
        TableRegs<uint64_t, 7 * 116> q_fac;
        q_quot.fetch(&K_QUOT[0][0], tid);
        q_cards.fetch(&K_CARD_ROWS[0][0], tid);
        q_take.fetch(K_ACT_TAKE, tid);
        q_give.fetch(K_ACT_GIVE, tid);
        q_rsv.fetch(K_ACT_RSV, tid);
        q_fac.fetch(&K_MASK_FACTORS[0][0], tid);
        const double recip = K_RECIP[min(tid, 8)];
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
        q_quot.put(&tabs.quot[0][0], tid);
        q_cards.put(&tabs.cards[0][0], tid);
        q_take.put(tabs.act_take, tid);
        q_give.put(tabs.act_give, tid);
        q_rsv.put(tabs.act_rsv, tid);
        q_fac.put(mfac, tid);
        if (tid < 9) tabs.recip[tid] = recip;
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
        if (on) {
            uint64_t f0, f1;
            uint32_t cc;
            bool bad;
            const int8_t *s = lds + l * ST;
            switch (w) {
                case 0: lane_predicates_part<N, 0>(s, pl[l], lim, f0, f1, cc, bad); break;
                case 1: lane_predicates_part<N, 1>(s, pl[l], lim, f0, f1, cc, bad); break;
                case 2: lane_predicates_part<N, 2>(s, pl[l], lim, f0, f1, cc, bad); break;
                default: lane_predicates_part<N, 3>(s, pl[l], lim, f0, f1, cc, bad); break;
            }
            pf0[w][l] = f0;
            if (w == 3) pf1[l] = f1;
            if (w == 2) pcond[l] = cc;
            pbad[w][l] = bad;
        }
        __builtin_amdgcn_s_setprio(0);
        lds_sync();
        // mask words w and w+4 of every live task (factorised words; boards outside the fast
        // domain take the exact predicates and the per-action descriptor words)
        if (on) {
            const bool bad = pbad[0][l] | pbad[1][l] | pbad[2][l] | pbad[3][l];
            if (bad) {
                const LanePred Q = lane_predicates_exact<N>(lds + l * ST, pl[l], lim);
                if (w == 0) { msk[l][0] = lane_mask_word<0>(Q); msk[l][4] = lane_mask_word<4>(Q); }
                else if (w == 1) { msk[l][1] = lane_mask_word<1>(Q); msk[l][5] = lane_mask_word<5>(Q); }
                else if (w == 2) { msk[l][2] = lane_mask_word<2>(Q); msk[l][6] = lane_mask_word<6>(Q); }
                else { msk[l][3] = lane_mask_word<3>(Q); }
            } else {
                const uint64_t F0 = pf0[0][l] | pf0[1][l] | pf0[2][l];
                const uint32_t C = pcond[l], lv = (uint32_t)pf1[l];
                if (w == 0) {
                    msk[l][0] = lane_mask_word_fast<0>(C, F0, lv, mfac);
                    msk[l][4] = lane_mask_word_fast<4>(C, F0, lv, mfac);
                } else if (w == 1) {
                    msk[l][1] = lane_mask_word_fast<1>(C, F0, lv, mfac);
                    msk[l][5] = lane_mask_word_fast<5>(C, F0, lv, mfac);
                } else if (w == 2) {
                    msk[l][2] = lane_mask_word_fast<2>(C, F0, lv, mfac);
                    msk[l][6] = lane_mask_word_fast<6>(C, F0, lv, mfac);
                } else {
                    msk[l][3] = lane_mask_word_fast<3>(C, F0, lv, mfac);
                }
            }
        }
        lds_sync();
        // the uniform prior over the input board's legal moves: once per active row, from the
        // first mask of its task 0 (pass alone when nothing else is legal). Block-uniform.
        if (t == 0 && pi_out) {
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
        // select: four lanes per task (task w*16 + l/4; lane q = l%4 holds mask words 2q, 2q+1):
        // quad-wide counts by DPP, then the lane whose words hold the drawn index finds its bit.
        // BUY_FIRST keeps only the buy bits of word 0 when there are any. Pass bit when nothing
        // is legal; the task is filed by move kind.
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
            const int c0 = __popcll(x0), c = c0 + __popcll(x1);
            const int k0 = quad_bcast<0>(c), k1 = quad_bcast<1>(c), k2 = quad_bcast<2>(c), k3 = quad_bcast<3>(c);
            const int cnt = k0 + k1 + k2 + k3;
            const int pre = (q > 0 ? k0 : 0) + (q > 1 ? k1 : 0) + (q > 2 ? k2 : 0);
            int a = -1;
            if (sel) {
                if (cnt == 0) {
                    if (q == 3) a = SPL_ACTIONS - 1;
                } else {
                    const int r = (int)(ud[b][0] * (double)cnt) - pre;
                    if (r >= 0 && r < c) {
                        const bool hi = r >= c0;
                        a = 128 * q + (hi ? 64 : 0) + kth_bit64(hi ? x1 : x0, hi ? r - c0 : r);
                    }
                }
            }
            if (a >= 0) {
                const int kind = move_kind_of(a);
                klist[kind][atomicAdd(&kcount[kind], 1)] = (uint32_t)b | (uint32_t)a << 8 | (uint32_t)pl[b] << 20;
            }
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
                const int r = (uint8_t)(bt(row(s, Lx::BANK), 6) + 1);   // the round after the move
                Chance ch{&ud[b][0], 0, 0, 0, 1, 0.0, false, tabs.view()};
                int nxt;
                switch (w) {
                    case MK_GEMS: nxt = make_move<N, MK_GEMS>(s, a, p, false, ch); break;
                    case MK_BUY: nxt = make_move<N, MK_BUY>(s, a, p, false, ch); break;
                    case MK_RESERVE: nxt = make_move<N, MK_RESERVE>(s, a, p, false, ch); break;
                    default: nxt = make_move<N, MK_BUY_RESERVED>(s, a, p, false, ch); break;
                }
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
            result[(size_t)(LIST ? erow[rr] : r0 + rr) * N + i] = sum / (float)P;
        }
    }
    if (w == 0) {
        const bool on = l < nb && act[l];
        if (steps_out && on) steps_out[LIST ? (size_t)myrow * P + (l - lrow * P) : (size_t)r0 * P + l] = nstep[l];
        const uint64_t open = __ballot(l < nb && live[l]);   // still playing after max_steps moves
        if (unfinished && open && l == 0) atomicAdd(unfinished, (int32_t)__popcll(open));
    }
}

inline bool ok_ctx(const spl_ctx *c) { return c && c->n >= 2 && c->n <= 4; }

// one launch of k_playout<N, SEQ, LIST>; a list launch is sized for B entries (the host cannot
// know the list's length: the workgroups past its end leave at once)
template <bool SEQ, bool LIST>
int launch_playout(const spl_ctx *c, int B, const int8_t *state, const int8_t *player, const uint8_t *active,
                   int policy, int playouts, int max_steps, uint64_t seed, uint32_t step0, uint32_t board_base,
                   float *result, float *pi_out, int32_t *steps_out, int32_t *unfinished, const int32_t *leaf_index,
                   const int32_t *leaf_count, const uint32_t *call_seq, void *hs) {
    const int rpw = PT / playouts;
    const dim3 grid((unsigned)(((long long)B + rpw - 1) / rpw));
#define SPL_PLAYOUT_LAUNCH(NP)                                                                            \
    hipLaunchKernelGGL((k_playout<NP, SEQ, LIST>), grid, dim3(THREADS), 0, (hipStream_t)hs, B, playouts,  \
                       state, player, active, pack_lim(c->token_limit, c->rules), policy, max_steps,      \
                       seed, step0, board_base, result, pi_out, steps_out, unfinished, leaf_index,        \
                       leaf_count, call_seq)
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
