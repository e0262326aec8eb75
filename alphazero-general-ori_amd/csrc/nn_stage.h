// nn_stage.h — the staged leaf buffer shared by k_leaf_mask (mcts.hip, the writer) and
// k_nn_forward (nnet.hip, the reader); layout in include/splendor_amd.h (spl_nn_stage_bytes).
// Both sides static_assert these constants against their own (Net<NP>::X0S, ML; Lay<N>::ROWS).
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

}  // namespace nnstage
