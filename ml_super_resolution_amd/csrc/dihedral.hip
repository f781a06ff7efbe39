// dihedral.hip -- the eight flips and transposes of an image batch in one launch (srx_dihedral_expand) and the average
// of their inverses in one launch (srx_dihedral_merge): the two ends of geometric self-ensemble inference.
//
// Both kernels are bound by HBM: expand reads x once and writes eight images, merge reads eight and writes one, and
// neither does arithmetic worth the name.  A workgroup owns one 32 x 32 pixel tile of x (of out).  The
// four images of the A group (k = 0..3, [H,W,C]) keep the tile's rows, so a tile row goes to global memory as one
// contiguous run of up to 32 C floats, forwards or with its pixels reversed.  In the four images of the B group
// (k = 4..7, [W,H,C]) the tile's COLUMNS are the contiguous runs: the tile crosses the LDS (dihedral.h: one pixel of
// padding per row, no bank conflict either way), so that global memory only ever sees such runs.  Every access is one
// float per lane: a pixel has 12 bytes at C = 3 and a row may start at any 4-byte address, and one dword per lane is
// 256 contiguous bytes per wave instruction, which streams at the rate of wider stores on this chip.
//
// Element offsets are 64-bit (size_t); tile-local indices are ints below 32 * 32 * 8.  C is a template argument: the
// split of a float index into (pixel, channel) divides by a constant.
#include "dihedral.h"

namespace srx {
namespace {

constexpr int kThreads = 256;          // expand
constexpr int kMergeThreads = 1024;    // merge: a thread keeps C running sums, not 4 C, across the four LDS passes

struct Tile {
    int n, row0, col0, th, tw;     // image; first row / column; valid rows / columns (1..32)
};
__device__ inline Tile this_tile(int H, int W, int tiles_y, int tiles_x) {
    unsigned blk = blockIdx.x;
    Tile t;
    const int tx = (int)(blk % (unsigned)tiles_x);
    blk /= (unsigned)tiles_x;
    const int ty = (int)(blk % (unsigned)tiles_y);
    t.n = (int)(blk / (unsigned)tiles_y);
    t.row0 = ty * kDihedralTile;
    t.col0 = tx * kDihedralTile;
    t.th = min(kDihedralTile, H - t.row0);
    t.tw = min(kDihedralTile, W - t.col0);
    return t;
}

template <int C>
__global__ __launch_bounds__(kThreads) void dihedral_expand_kernel(const float* __restrict__ x, float* __restrict__ a,
                                                                   float* __restrict__ b, int N, int H, int W, int tiles_y,
                                                                   int tiles_x) {
    constexpr int T = kDihedralTile, RF = T * C, P = dihedral_pitch(C), E = T * RF;
    __shared__ float tile[T * P];
    const int t = threadIdx.x;
    const Tile tl = this_tile(H, W, tiles_y, tiles_x);
    const int row0 = tl.row0, col0 = tl.col0, th = tl.th, tw = tl.tw;
    const size_t WC = (size_t)W * C, HC = (size_t)H * C, img = (size_t)H * WC, group = (size_t)N * img;

    // the tile of x, row by row: tile[i][f], f = pixel * C + channel
    const float* xin = x + tl.n * img + (size_t)row0 * WC + (size_t)col0 * C;
#pragma unroll 4
    for (int e = t; e < E; e += kThreads) {
        const int i = e / RF, f = e - i * RF;
        if (i < th && f < tw * C) tile[i * P + f] = xin[(size_t)i * WC + f];
    }
    __syncthreads();

    // A group: a tile row stays a row.  k = 0 as it is, 1 pixels reversed, 2 rows reversed, 3 both.
    float* a0 = a + tl.n * img;
#pragma unroll 2
    for (int e = t; e < E; e += kThreads) {
        const int i = e / RF, f = e - i * RF, p = f / C, c = f - p * C;
        if (i < th && f < tw * C) {
            const float fw = tile[i * P + f], bw = tile[i * P + (tw - 1 - p) * C + c];
            const size_t r_up = (size_t)(row0 + i) * WC, r_dn = (size_t)(H - 1 - row0 - i) * WC;
            const size_t c_fw = (size_t)col0 * C + f, c_bw = (size_t)(W - col0 - tw + p) * C + c;
            a0[r_up + c_fw] = fw;
            a0[group + r_up + c_bw] = bw;
            a0[2 * group + r_dn + c_fw] = fw;
            a0[3 * group + r_dn + c_bw] = bw;
        }
    }
    // B group, images [W,H,C]: tile column j is (a piece of) row col0 + j.  k = 4 the transpose, 5 its pixels reversed
    // (tile rows from the bottom), 6 its rows reversed, 7 both.
    float* b0 = b + tl.n * img;
#pragma unroll 2
    for (int e = t; e < E; e += kThreads) {
        const int j = e / RF, g = e - j * RF, q = g / C, c = g - q * C;
        if (j < tw && g < th * C) {
            const float fw = tile[q * P + j * C + c], bw = tile[(th - 1 - q) * P + j * C + c];
            const size_t r_up = (size_t)(col0 + j) * HC, r_dn = (size_t)(W - 1 - col0 - j) * HC;
            const size_t c_fw = (size_t)row0 * C + g, c_bw = (size_t)(H - row0 - th + q) * C + c;
            b0[r_up + c_fw] = fw;
            b0[group + r_up + c_bw] = bw;
            b0[2 * group + r_dn + c_fw] = fw;
            b0[3 * group + r_dn + c_bw] = bw;
        }
    }
}

// out = (((((((U0 + U1) + U2) + U3) + U4) + U5) + U6) + U7) * 0.125f, U_k the inverse transform of group k: the same
// places expand writes, read.  A thread of the 1024 keeps the running sums of its E / 1024 = C tile elements in
// registers (with 256 threads the 4 C sums and their addresses spill from C = 6 on).  The A group is read straight from
// global memory (runs of a tile row), then the B group's four tiles cross the LDS one after the other, in the order of
// the sum.
template <int C>
__global__ __launch_bounds__(kMergeThreads) void dihedral_merge_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  float* __restrict__ out, int N, int H, int W, int tiles_y,
                                                                  int tiles_x) {
    constexpr int T = kDihedralTile, RF = T * C, P = dihedral_pitch(C), E = T * RF, M = E / kMergeThreads;
    static_assert(E % kMergeThreads == 0, "every thread owns the same number of tile elements");
    __shared__ float tile[T * P];
    const int t = threadIdx.x;
    const Tile tl = this_tile(H, W, tiles_y, tiles_x);
    const int row0 = tl.row0, col0 = tl.col0, th = tl.th, tw = tl.tw;
    const size_t WC = (size_t)W * C, HC = (size_t)H * C, img = (size_t)H * WC, group = (size_t)N * img;

    float acc[M];
    const float* a0 = a + tl.n * img;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int e = t + m * kMergeThreads, i = e / RF, f = e - i * RF, p = f / C, c = f - p * C;
        acc[m] = 0.0f;
        if (i < th && f < tw * C) {
            const size_t r_up = (size_t)(row0 + i) * WC, r_dn = (size_t)(H - 1 - row0 - i) * WC;
            const size_t c_fw = (size_t)col0 * C + f, c_bw = (size_t)(W - 1 - col0 - p) * C + c;
            float s = a0[r_up + c_fw];
            s = s + a0[group + r_up + c_bw];
            s = s + a0[2 * group + r_dn + c_fw];
            s = s + a0[3 * group + r_dn + c_bw];
            acc[m] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // group 4 + k, image [W,H,C]: rows col0.. (k & 2: counted from the far end), floats from row0 * C (k & 1: from
        // the far end) -- the piece expand wrote from this tile, staged as tile[j][g] in the order it lies in memory
        const bool far_px = (k & 1) != 0, far_row = (k & 2) != 0;
        const float* src = b + k * group + tl.n * img + (size_t)(far_row ? W - col0 - tw : col0) * HC +
                           (size_t)(far_px ? H - row0 - th : row0) * C;
        if (k) __syncthreads();       // the sums of the tile before are taken
#pragma unroll 4
        for (int e = t; e < E; e += kMergeThreads) {
            const int j = e / RF, g = e - j * RF;
            if (j < tw && g < th * C) tile[j * P + g] = src[(size_t)j * HC + g];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int e = t + m * kMergeThreads, i = e / RF, f = e - i * RF, p = f / C, c = f - p * C;
            if (i < th && f < tw * C) {
                const int jj = far_row ? tw - 1 - p : p, ii = far_px ? th - 1 - i : i;
                acc[m] = acc[m] + tile[jj * P + ii * C + c];
            }
        }
    }
    float* o = out + tl.n * img + (size_t)row0 * WC + (size_t)col0 * C;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int e = t + m * kMergeThreads, i = e / RF, f = e - i * RF;
        if (i < th && f < tw * C) o[(size_t)i * WC + f] = acc[m] * 0.125f;
    }
}

template <int C>
hipError_t expand_c(const float* x, float* a, float* b, int N, int H, int W, const DihedralGrid& g, hipStream_t s) {
    hipLaunchKernelGGL(dihedral_expand_kernel<C>, dim3((unsigned)g.blocks), dim3(kThreads), 0, s, x, a, b, N, H, W, g.tiles_y,
                       g.tiles_x);
    return hipGetLastError();
}
template <int C>
hipError_t merge_c(const float* a, const float* b, float* out, int N, int H, int W, const DihedralGrid& g, hipStream_t s) {
    hipLaunchKernelGGL(dihedral_merge_kernel<C>, dim3((unsigned)g.blocks), dim3(kMergeThreads), 0, s, a, b, out, N, H, W, g.tiles_y,
                       g.tiles_x);
    return hipGetLastError();
}

}  // namespace

// The callers (srx_api.hip) have checked N, H, W >= 1, C in 1..8 and the grid limit.
hipError_t launch_dihedral_expand(const float* x, float* a, float* b, int N, int H, int W, int C, hipStream_t s) {
    const DihedralGrid g = dihedral_grid(N, H, W);
    switch (C) {
        case 1: return expand_c<1>(x, a, b, N, H, W, g, s);
        case 2: return expand_c<2>(x, a, b, N, H, W, g, s);
        case 3: return expand_c<3>(x, a, b, N, H, W, g, s);
        case 4: return expand_c<4>(x, a, b, N, H, W, g, s);
        case 5: return expand_c<5>(x, a, b, N, H, W, g, s);
        case 6: return expand_c<6>(x, a, b, N, H, W, g, s);
        case 7: return expand_c<7>(x, a, b, N, H, W, g, s);
        case 8: return expand_c<8>(x, a, b, N, H, W, g, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_dihedral_merge(const float* a, const float* b, float* out, int N, int H, int W, int C, hipStream_t s) {
    const DihedralGrid g = dihedral_grid(N, H, W);
    switch (C) {
        case 1: return merge_c<1>(a, b, out, N, H, W, g, s);
        case 2: return merge_c<2>(a, b, out, N, H, W, g, s);
        case 3: return merge_c<3>(a, b, out, N, H, W, g, s);
        case 4: return merge_c<4>(a, b, out, N, H, W, g, s);
        case 5: return merge_c<5>(a, b, out, N, H, W, g, s);
        case 6: return merge_c<6>(a, b, out, N, H, W, g, s);
        case 7: return merge_c<7>(a, b, out, N, H, W, g, s);
        case 8: return merge_c<8>(a, b, out, N, H, W, g, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace srx
