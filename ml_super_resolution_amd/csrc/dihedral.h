// dihedral.h -- internal: what the host side (srx_api.hip: srx_dihedral_expand, srx_dihedral_merge) and the two kernels
// of dihedral.hip must agree on: the tile, the LDS pitch, the grid and the launchers' weak declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srx.h"

namespace srx {

constexpr int kDihedralTile = 32;         // pixels of a tile's side: one workgroup moves a 32 x 32 pixel tile of x / out
constexpr int kDihedralMaxC = SRX_DIHEDRAL_MAX_C;
constexpr long long kDihedralMaxTiles = 0x7fffffffLL;     // one workgroup per (image, tile): the grid's x limit

// Floats of one LDS tile row: 32 pixels and one more.  33 C = C (mod 32), so float (i, c) of a tile COLUMN, at
// i * pitch + c, falls on bank (i C + c + const) mod 32: the 32 lanes of an access group, which walk (i, c) in that
// order when they write a transposed row, take 32 different banks.  A tile ROW is contiguous anyway.
__host__ __device__ constexpr int dihedral_pitch(int C) { return (kDihedralTile + 1) * C; }
__host__ __device__ constexpr int dihedral_lds_bytes(int C) { return kDihedralTile * dihedral_pitch(C) * (int)sizeof(float); }
static_assert(dihedral_lds_bytes(kDihedralMaxC) <= 64 * 1024, "the tile stays within the LDS every launch may use");

// tiles of one image [H,W,C]; the grid is N * tiles_y * tiles_x workgroups, image-major, then tile rows
struct DihedralGrid {
    int tiles_y, tiles_x;
    long long blocks;
};
inline DihedralGrid dihedral_grid(int N, int H, int W) {
    DihedralGrid g;
    g.tiles_y = (int)(((long long)H + kDihedralTile - 1) / kDihedralTile);
    g.tiles_x = (int)(((long long)W + kDihedralTile - 1) / kDihedralTile);
    const long long per_image = (long long)g.tiles_y * g.tiles_x;      // < 2^54
    g.blocks = per_image > kDihedralMaxTiles / N ? -1 : per_image * N;  // -1: the grid limit is exceeded
    return g;
}

// One launch each.  Weak references, as launch_image_scores: a host-only build of srx_api.hip without the kernel units
// links, and the two entry points refuse.
__attribute__((weak)) hipError_t launch_dihedral_expand(const float* x, float* a, float* b, int N, int H, int W, int C, hipStream_t s);
__attribute__((weak)) hipError_t launch_dihedral_merge(const float* a, const float* b, float* out, int N, int H, int W, int C, hipStream_t s);

}  // namespace srx
