// nn_stage.h — the staged leaf buffer shared by k_leaf_mask (mcts.hip, the writer) and
// k_nn_forward (nnet.hip, the reader); layout in include/splendor_amd.h (spl_nn_stage_bytes).
// Both sides static_assert these constants against their own (Net<NP>::X0S, ML; Lay<N>::ROWS).
// Also the scan of k_leaf_mask's segmented leaf list (leaf_list_scan), for its readers
// k_nn_forward and k_playout (playout.hip). Include after <hip/hip_runtime.h>.
#pragma once
#include <cstddef>

namespace nnstage {

constexpr int TILE = 32;                                   // leaves per network tile (nnet.hip ML)
__host__ __device__ constexpr int rows(int np) { return 32 + 10 * np + np * np; }
// int8 stride of one (column, leaf) run of the tile image: the board's rows padded to 8, an odd
// number of dwords (LDS banks)
__host__ __device__ constexpr int x0s(int np) {
    const int kp = (rows(np) + 7) / 8 * 8;
    return (kp / 4) % 2 ? kp : kp + 4;
}
__host__ __device__ constexpr int tile_bytes(int np) { return 7 * TILE * x0s(np); }
__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15) / 16 * 16; }
// byte offsets of header (i32 total, 12 bytes reserved), rows[B] i32, mask[B][7] u64,
// x[ceil(B / TILE)][7][TILE][x0s] int8
constexpr size_t ROWS_OFF = 16;
__host__ __device__ constexpr size_t mask_off(int B) { return align16(ROWS_OFF + 4 * (size_t)B); }
__host__ __device__ constexpr size_t x_off(int B) { return align16(mask_off(B) + 56 * (size_t)B); }
__host__ __device__ constexpr size_t bytes(int np, int B) {
    return x_off(B) + (size_t)((B + TILE - 1) / TILE) * tile_bytes(np);
}
static_assert(tile_bytes(2) % 16 == 0 && tile_bytes(3) % 16 == 0 && tile_bytes(4) % 16 == 0, "16-byte tile copies");

// The search's NN leaves as k_leaf_mask lists them (ABI 11): segment j (trees 64 j .. 64 j + 63)
// has count[j] leaves at idx[64 j ..]; the list is their concatenation in segment order. The
// scan of the list's two readers, k_nn_forward's indexed mode (32 leaves per tile) and
// k_playout's list mode (64 task slots per workgroup).
// Wave-collective, registers only unless `slot` is given: returns the list's length, and with
// slot / offv (SLOTS ints each, the calling wave's own) lane i < SLOTS gets the idx position of
// list entry e0 + i in `pos` (meaningful for entries below the length). A lane holds SEGS
// consecutive segments' counts (clamped to 0 .. 64; VEC16: 16-byte loads of 16-byte aligned
// counts) and one DPP scan gives every segment's first entry, 64 SEGS segments per pass; each
// segment that reaches into [e0, e0 + SLOTS) marks the slot where it starts (and 64 j - start
// in offv), and a prefix maximum over the slots gives every slot its segment.
template <int SLOTS, int SEGS, bool VEC16>
__device__ __forceinline__ int leaf_list_scan(const int32_t *__restrict__ count, int nseg, int e0, int *slot, int *offv,
                                              int &pos) {
    static_assert(SLOTS == 32 || SLOTS == 64, "the prefix maximum covers two or four DPP rows");
    static_assert(!VEC16 || SEGS % 4 == 0, "16-byte loads: four counts each");
    const int lane = threadIdx.x & 63;
    if (slot && lane < SLOTS) slot[lane] = -1;
    int base = 0;
    for (int c0 = 0; c0 < nseg; c0 += SEGS * 64) {
        const int j0 = c0 + SEGS * lane;
        int v[SEGS];
        if (VEC16 && j0 + SEGS <= nseg) {
#pragma unroll
            for (int q = 0; q < SEGS; q += 4) {
                const int4 a = *reinterpret_cast<const int4 *>(count + j0 + q);
                v[q] = a.x; v[q + 1] = a.y; v[q + 2] = a.z; v[q + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < SEGS; q++) v[q] = count[min(j0 + q, nseg - 1)];
        }
        int own = 0;
#pragma unroll
        for (int q = 0; q < SEGS; q++) {
            v[q] = min(max(v[q], 0), j0 + q < nseg ? 64 : 0);
            own += v[q];
        }
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
            for (int q = 0; q < SEGS; q++) {
                if (v[q] > 0 && ex + v[q] > e0 && ex < e0 + SLOTS) {
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
        int f = lane < SLOTS ? slot[lane] : -1;          // prefix maximum over slots 0 .. SLOTS - 1
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x111, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x112, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x114, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x118, 0xf, 0xf, false));
        f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x142, 0xa, 0xf, false));
        if (SLOTS > 32) f = max(f, __builtin_amdgcn_update_dpp(-1, f, 0x143, 0xc, 0xf, false));
        if (f >= 0) pos = e0 + lane + offv[f];
    }
    return base;
}

}  // namespace nnstage
