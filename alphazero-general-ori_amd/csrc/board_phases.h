// board_phases.h — the phases shared by the kernels that keep a workgroup's boards in LDS, a
// lane per board, four waves per workgroup: k_rollout (splendor_env.hip), k_playout
// (playout.hip) and k_leaf_mask (mcts.hip). Each kernel keeps what is its own around the calls
// (which lanes are on, wave priorities, probes, barriers, outputs); the rule logic underneath is
// splendor_device.h's.
//   prologue  StageRegs / TabsRegs / BoardRegs: every global load issued before the first LDS
//             store (a loop of load -> store pairs waits one round trip per iteration)
//   preds     phase_predicates: part w of every board's predicate set in wave w
//   mask      phase_mask_words: mask words w, w+4 in wave w
//   select    quad_select: four lanes per board draw one legal action; file_move
//   move      lane_move_of_kind: wave k makes the moves of kind k
#pragma once
#include "splendor_device.h"

namespace spl {

constexpr int MASK_FACTOR_WORDS = 7 * 116;   // K_MASK_FACTORS (lane_mask_word_fast)

// v of lane I of this lane's quad (DPP quad_perm broadcast; every lane must be active)
template <int I>
__device__ __forceinline__ int quad_bcast(int v) {
    return __builtin_amdgcn_update_dpp(v, v, I | I << 2 | I << 4 | I << 6, 0xF, 0xF, false);
}
// a board's LDS slot: 8-byte rows at an odd qword stride (conflict-free lane-per-board
// ds_read_b64 / ds_write_b64)
template <int N>
struct RolloutLds {
    static constexpr int STRIDE = (Lay<N>::ROWS % 2 ? Lay<N>::ROWS : Lay<N>::ROWS + 1) * 8;
};

// ------------------------------------------------------------------ prologue
// COUNT elements of a table held in registers across the workgroup's THREADS threads:
// fetch() issues every load (clamped indices, no branch, so they all go out back to back),
// put() stores them into LDS after the other fetches
template <class T, int COUNT, int THREADS>
struct StageRegs {
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

// the transition tables (TabsLds) and the mask factors of the move loops
template <int THREADS>
struct TabsRegs {
    StageRegs<double, 41 * 9, THREADS> quot;
    StageRegs<uint64_t, 240, THREADS> cards;
    StageRegs<uint64_t, 409, THREADS> take, give;
    StageRegs<int8_t, 409, THREADS> rsv;
    StageRegs<uint64_t, MASK_FACTOR_WORDS, THREADS> fac;
    double recip;
    __device__ __forceinline__ void fetch(int tid) {
        quot.fetch(&K_QUOT[0][0], tid);
        cards.fetch(&K_CARD_ROWS[0][0], tid);
        take.fetch(K_ACT_TAKE, tid);
        give.fetch(K_ACT_GIVE, tid);
        rsv.fetch(K_ACT_RSV, tid);
        fac.fetch(&K_MASK_FACTORS[0][0], tid);
        recip = K_RECIP[min(tid, 8)];
    }
    __device__ __forceinline__ void put(TabsLds &tabs, uint64_t *mfac, int tid) const {
        quot.put(&tabs.quot[0][0], tid);
        cards.put(&tabs.cards[0][0], tid);
        take.put(tabs.act_take, tid);
        give.put(tabs.act_give, tid);
        rsv.put(tabs.act_rsv, tid);
        fac.put(mfac, tid);
        if (tid < 9) tabs.recip[tid] = recip;
    }
};

// the workgroup's nb <= RB consecutive HBM boards (g: the first) into their LDS slots. Boards
// of whole 4-row quads are fetched into registers (clamped index: every load is valid) and put
// later; the others (3 players) go byte by byte inside put().
template <int N, int RB, int THREADS>
struct BoardRegs {
    using Cv = Conv<N>;
    static constexpr int IT = Cv::QUAD ? (RB * Cv::UNITS + THREADS - 1) / THREADS : 1;
    uint32_t d[IT][7];
    __device__ __forceinline__ void fetch(const int8_t *g, int nb, int tid) {
        if constexpr (Cv::QUAD) {
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const int i = min(tid + k * THREADS, nb * Cv::UNITS - 1), b = i / Cv::UNITS, u = i - b * Cv::UNITS;
                const uint32_t *q = reinterpret_cast<const uint32_t *>(g + (size_t)b * Lay<N>::S) + 7 * u;
#pragma unroll
                for (int j = 0; j < 7; j++) d[k][j] = q[j];
            }
        }
    }
    __device__ __forceinline__ void put(int8_t *lds, const int8_t *g, int nb, int tid) const {
        constexpr int ST = RolloutLds<N>::STRIDE;
        if constexpr (Cv::QUAD) {
#pragma unroll
            for (int k = 0; k < IT; k++) {
                const int i = tid + k * THREADS, b = i / Cv::UNITS, u = i - b * Cv::UNITS;
                if (i < nb * Cv::UNITS) quad_rows_put(d[k], reinterpret_cast<uint64_t *>(lds + b * ST) + 4 * u);
            }
        } else {
            for (int i = tid; i < nb * Cv::UNITS; i += THREADS) {
                const int b = i / Cv::UNITS, u = i - b * Cv::UNITS;
                Cv::load(lds + b * ST, g + (size_t)b * Lay<N>::S, u);
            }
        }
    }
};

// ------------------------------------------------------------------ predicates, mask words
// what the predicate phase leaves for the mask phase, per board
template <int RB>
struct PredLds {
    uint64_t f0[4][RB], f1[RB];
    uint32_t cond[RB];
    uint8_t bad[4][RB];
    // board l is outside the fast domain (a negative byte): it takes the exact predicates
    __device__ __forceinline__ bool any_bad(int l) const { return bad[0][l] | bad[1][l] | bad[2][l] | bad[3][l]; }
};

// wave w computes part w of board l's predicate set for player p (lane_predicates_part: cards
// 0-5 / cards 6-11 / reserved cards, decks, conditions / colour levels)
template <int N, int RB>
__device__ __forceinline__ void phase_predicates(int w, int l, const int8_t *s, int p, int lim, PredLds<RB> &pr) {
    uint64_t f0, f1;
    uint32_t cc;
    bool bad;
    switch (w) {
        case 0: lane_predicates_part<N, 0>(s, p, lim, f0, f1, cc, bad); break;
        case 1: lane_predicates_part<N, 1>(s, p, lim, f0, f1, cc, bad); break;
        case 2: lane_predicates_part<N, 2>(s, p, lim, f0, f1, cc, bad); break;
        default: lane_predicates_part<N, 3>(s, p, lim, f0, f1, cc, bad); break;
    }
    pr.f0[w][l] = f0;
    if (w == 3) pr.f1[l] = f1;
    if (w == 2) pr.cond[l] = cc;
    pr.bad[w][l] = bad;
}

// after a barrier: wave w writes words w and w+4 of board l's mask into m[0..6] — factorised
// words from the card predicates, condition bits and colour levels (mfac: K_MASK_FACTORS in
// LDS); a board outside the fast domain takes the exact predicates and the per-action
// descriptor words. The pass bit is not included.
template <int N, int RB>
__device__ __forceinline__ void phase_mask_words(int w, int l, const int8_t *s, int p, int lim, const PredLds<RB> &pr,
                                                 const uint64_t *mfac, uint64_t *m) {
    if (pr.any_bad(l)) {
        const LanePred P = lane_predicates_exact<N>(s, p, lim);
        if (w == 0) { m[0] = lane_mask_word<0>(P); m[4] = lane_mask_word<4>(P); }
        else if (w == 1) { m[1] = lane_mask_word<1>(P); m[5] = lane_mask_word<5>(P); }
        else if (w == 2) { m[2] = lane_mask_word<2>(P); m[6] = lane_mask_word<6>(P); }
        else { m[3] = lane_mask_word<3>(P); }
    } else {
        const uint64_t F0 = pr.f0[0][l] | pr.f0[1][l] | pr.f0[2][l];
        const uint32_t C = pr.cond[l], lv = (uint32_t)pr.f1[l];
        if (w == 0) {
            m[0] = lane_mask_word_fast<0>(C, F0, lv, mfac);
            m[4] = lane_mask_word_fast<4>(C, F0, lv, mfac);
        } else if (w == 1) {
            m[1] = lane_mask_word_fast<1>(C, F0, lv, mfac);
            m[5] = lane_mask_word_fast<5>(C, F0, lv, mfac);
        } else if (w == 2) {
            m[2] = lane_mask_word_fast<2>(C, F0, lv, mfac);
            m[6] = lane_mask_word_fast<6>(C, F0, lv, mfac);
        } else {
            m[3] = lane_mask_word_fast<3>(C, F0, lv, mfac);
        }
    }
}

// ------------------------------------------------------------------ select
// Four lanes per board: lane q of the quad holds mask words 2q (x0) and 2q+1 (x1; 0 for q = 3),
// already filtered by the caller's policy. Quad-wide counts by DPP, then the lane whose words
// hold bit (int)(u cnt) of the quad's cnt set bits finds it, so no lane walks all seven words:
// `a` is the action in that lane and -1 in the others (in all four when cnt = 0: the caller
// sets the pass bit). Every lane of the wave must be active.
struct QuadPick {
    int a, cnt;
};
__device__ __forceinline__ QuadPick quad_select(uint64_t x0, uint64_t x1, int q, double u) {
    const int c0 = __popcll(x0), c = c0 + __popcll(x1);
    const int k0 = quad_bcast<0>(c), k1 = quad_bcast<1>(c), k2 = quad_bcast<2>(c), k3 = quad_bcast<3>(c);
    const int cnt = k0 + k1 + k2 + k3;
    const int pre = (q > 0 ? k0 : 0) + (q > 1 ? k1 : 0) + (q > 2 ? k2 : 0);
    int a = -1;
    if (cnt != 0) {
        const int r = (int)(u * (double)cnt) - pre;
        if (r >= 0 && r < c) {
            const bool hi = r >= c0;
            a = 128 * q + (hi ? 64 : 0) + kth_bit64(hi ? x1 : x0, hi ? r - c0 : r);
        }
    }
    return QuadPick{a, cnt};
}

// board b's move a by player p, filed under its kind for the move phase:
// klist[kind][..] = board | action << 8 | player << 20
template <int RB>
__device__ __forceinline__ void file_move(uint32_t (*klist)[RB], int *kcount, int b, int a, int p) {
    const int kind = move_kind_of(a);
    klist[kind][atomicAdd(&kcount[kind], 1)] = (uint32_t)b | (uint32_t)a << 8 | (uint32_t)p << 20;
}

// ------------------------------------------------------------------ move
// Wave `kind` makes a filed move of its kind on board s (one pipeline specialisation per wave,
// so no wave carries the stages of other kinds); the chance draws continue the board's step
// stream at draw 1 (ud: its draws 0..3). Returns the next player; round = the round after the
// move (check_end_round).
template <int N>
__device__ __forceinline__ int lane_move_of_kind(int kind, int8_t *s, int a, int p, const double *ud, const Tabs &tab,
                                                 int &round) {
    round = (uint8_t)(bt(row(s, Lay<N>::BANK), 6) + 1);
    Chance ch{ud, 0, 0, 0, 1, 0.0, false, tab};
    switch (kind) {
        case MK_GEMS: return make_move<N, MK_GEMS>(s, a, p, false, ch);
        case MK_BUY: return make_move<N, MK_BUY>(s, a, p, false, ch);
        case MK_RESERVE: return make_move<N, MK_RESERVE>(s, a, p, false, ch);
        default: return make_move<N, MK_BUY_RESERVED>(s, a, p, false, ch);
    }
}

}  // namespace spl
