// image_scores.hip -- PSNR and SSIM of up to four candidates against one reference image, two launches per call.
//
// The reference scores every evaluated image with tf.image.psnr and tf.image.ssim, one call per pair
// (vdsr/vdsr/experiment_evaluate.py:57-60: (hd, sd) and (hd, sr); espcn/espcn/experiment_test.py:32-55 after mapping
// to [0,1], clipping and, for 'y', keeping Y of the sub-pixel arrangement).  Here one call scores all candidates of an
// image against its reference and shares the reference's loads and window moments among them.
//
// image_scores_kernel: one workgroup (256 threads, wave64) owns a tile of kScoresTileH x kScoresTileW window positions of
// one image; a row is RL = We * Ce floats with tap stride Ce (image_scores.h).  Everything between the global loads and
// the two partial sums per candidate lives in LDS:
//   g        the 11 window weights, formed as ssim_partial_kernel forms them
//   A        the (tile + 10 rows, + 10 Ce columns) halo region of ref, front end applied during the load; zero outside
//            the image
//   H0, H1   horizontal 11-tap pass of A: mu, E[a^2]; the vertical pass leaves ref's two moments of each thread's
//            window positions in registers -- formed once for all candidates
//   then per candidate k, in turn:
//   B        its halo region, loaded as A was; the squared error against A is taken in the same pass over the elements
//            the tile owns: each element of the effective image belongs to the tile of its (row / tile_h, column /
//            tile_w), and the last tile row and column also own the ten trailing rows and 10 Ce trailing columns
//   H0..H2   horizontal pass of B: mu, E[b^2], E[ab]; the vertical pass forms the SSIM value of each window position
//            inside the image and adds it up
//   the workgroup's two sums go to its own slot of `scratch` (plain vector stores; no atomics, no communication
//   between workgroups; every slot the finish step reads is written on every call).
// 2 + 3 n_cand moment planes in all.  Every LDS slot a step reads was written by the step before it in full, so the
// result does not depend on what the LDS held (SRX_POISON_LDS).  A candidate's arithmetic does not depend on the other
// candidates: its numbers are the same bits alone and as slot k of four.
//
// image_scores_finish_kernel: one workgroup per (candidate, image) adds the image's slots in a fixed order in double, as
// ssim_finish_kernel does, and writes psnr (srx_psnr's formula: +inf for identical images) and the mean SSIM.
#include "image_scores.h"
#include "lds_launch.h"

namespace srx {

namespace {

__device__ __forceinline__ float scores_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the effective value at flat column x of an input row: unit_clip first, then the colour space
__device__ __forceinline__ float scores_unit(float v, int unit_clip) {
#pragma clang fp contract(off)
    if (unit_clip) {
        const float t = v * 0.5f;               // two roundings, as srx_affine
        v = fminf(fmaxf(t + 0.5f, 0.f), 1.f);
    }
    return v;
}
__device__ __forceinline__ float scores_load(const float* __restrict__ row, int x, int y_space, int unit_clip) {
#pragma clang fp contract(off)
    if (!y_space) return scores_unit(row[x], unit_clip);
    const float* p = row + 3 * (size_t)x;
    const float r = scores_unit(p[0], unit_clip), g = scores_unit(p[1], unit_clip), b = scores_unit(p[2], unit_clip);
    return (0.299f * r + 0.587f * g) + 0.114f * b;
}

}  // namespace

__global__ __launch_bounds__(256) void image_scores_kernel(const ImageScoresArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds_scores[];
    const ScoresLds L = scores_lds(a.Ce);
    float* gw = lds_scores + L.g;
    float* A = lds_scores + L.A;
    float* B = lds_scores + L.B;
    float* H0 = lds_scores + L.H0;
    float* H1 = lds_scores + L.H1;
    float* H2 = lds_scores + L.H2;
    float* red = lds_scores + L.red;
    const int t = threadIdx.x;
    const int Ce = a.Ce, pitch = scores_pitch(Ce);
    const int tiles = a.tiles_y * a.tiles_x;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int n = blockIdx.y;
    const int row0 = ty * kScoresTileH, col0 = tx * kScoresTileW;
    const bool last_y = ty == a.tiles_y - 1, last_x = tx == a.tiles_x - 1;
    const int OH = a.H - 10, OW = a.RL - 10 * Ce;
    const size_t image = (size_t)n * a.H * a.row_in;

    if (t < 11) {
        float sum = 0.f;
        for (int i = 0; i < 11; ++i) sum += __expf(-(float)((i - 5) * (i - 5)) / (2.0f * 1.5f * 1.5f));
        const int d = t - 5;
        gw[t] = __expf(-(float)(d * d) / (2.0f * 1.5f * 1.5f)) / sum;
    }
    // the halo region of ref
    {
        const float* img = a.ref + image;
        int r = 0, c = t;
        for (int o = t; o < kScoresHaloH * pitch; o += 256, c += 256) {
            while (c >= pitch) { c -= pitch; ++r; }         // (row, column) of o without a division: pitch >= 138
            const int gr = row0 + r, gc = col0 + c;
            A[o] = (gr < a.H && gc < a.RL) ? scores_load(img + (size_t)gr * a.row_in, gc, a.y_space, a.unit_clip) : 0.f;
        }
    }
    __syncthreads();
    float g[11];
#pragma unroll
    for (int j = 0; j < 11; ++j) g[j] = gw[j];
    // horizontal pass of ref
    for (int o = t; o < kScoresHaloH * kScoresTileW; o += 256) {
        const int r = o / kScoresTileW, x = o - r * kScoresTileW;
        const float* pa = A + r * pitch + x;
        float xa = 0.f, xaa = 0.f;
#pragma unroll
        for (int j = 0; j < 11; ++j) {
            const float va = pa[j * Ce], w = g[j];
            xa += w * va; xaa += w * va * va;
        }
        H0[o] = xa; H1[o] = xaa;
    }
    __syncthreads();
    // vertical pass of ref: thread t owns the window positions (rows 4 q .. 4 q + 3, column x) of its two items
    float mu_a[2][4], e_aa[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int item = t + k * 256, x = item % kScoresTileW, q = item / kScoresTileW;
        float v0[14], v1[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) {
            v0[i] = H0[(4 * q + i) * kScoresTileW + x];
            v1[i] = H1[(4 * q + i) * kScoresTileW + x];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ma = 0.f, saa = 0.f;
#pragma unroll
            for (int i = 0; i < 11; ++i) { ma += g[i] * v0[r + i]; saa += g[i] * v1[r + i]; }
            mu_a[k][r] = ma; e_aa[k][r] = saa;
        }
    }

    for (int cand = 0; cand < a.n_cand; ++cand) {
        // the candidate's halo region, and the squared error of the elements this tile owns.  B was last read by the
        // horizontal pass of the candidate before, which every thread left at a barrier.
        float se = 0.f;
        {
            const float* img = a.cand[cand] + image;
            int r = 0, c = t;
            for (int o = t; o < kScoresHaloH * pitch; o += 256, c += 256) {
                while (c >= pitch) { c -= pitch; ++r; }
                const int gr = row0 + r, gc = col0 + c;
                float v = 0.f;
                if (gr < a.H && gc < a.RL) {
                    v = scores_load(img + (size_t)gr * a.row_in, gc, a.y_space, a.unit_clip);
                    if ((r < kScoresTileH || last_y) && (c < kScoresTileW || last_x)) {
                        const float d = A[o] - v;
                        se += d * d;
                    }
                }
                B[o] = v;
            }
        }
        __syncthreads();        // also: every thread has left the vertical pass that read H0 .. H2
        for (int o = t; o < kScoresHaloH * kScoresTileW; o += 256) {
            const int r = o / kScoresTileW, x = o - r * kScoresTileW;
            const float* pa = A + r * pitch + x;
            const float* pb = B + r * pitch + x;
            float xb = 0.f, xbb = 0.f, xab = 0.f;
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                const float va = pa[j * Ce], vb = pb[j * Ce], w = g[j];
                xb += w * vb; xbb += w * vb * vb; xab += w * va * vb;
            }
            H0[o] = xb; H1[o] = xbb; H2[o] = xab;
        }
        __syncthreads();
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int item = t + k * 256, x = item % kScoresTileW, q = item / kScoresTileW;
            float v0[14], v1[14], v2[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) {
                v0[i] = H0[(4 * q + i) * kScoresTileW + x];
                v1[i] = H1[(4 * q + i) * kScoresTileW + x];
                v2[i] = H2[(4 * q + i) * kScoresTileW + x];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mb = 0.f, sbb = 0.f, sab = 0.f;
#pragma unroll
                for (int i = 0; i < 11; ++i) { mb += g[i] * v0[r + i]; sbb += g[i] * v1[r + i]; sab += g[i] * v2[r + i]; }
                // TF's _ssim_per_channel: luminance * contrast-structure (as ssim_partial_kernel)
                const float ma = mu_a[k][r], saa = e_aa[k][r];
                const float num0 = 2.0f * ma * mb, den0 = ma * ma + mb * mb;
                const float lum = (num0 + a.c1) / (den0 + a.c1);
                const float cs = (2.0f * sab - num0 + a.c2) / (saa + sbb - den0 + a.c2);
                if (row0 + 4 * q + r < OH && col0 + x < OW) acc += lum * cs;
            }
        }
        // the workgroup's two sums, in a fixed order; red was last read before the barriers above
        se = scores_wave_sum(se);
        acc = scores_wave_sum(acc);
        if ((t & 63) == 0) { red[2 * (t >> 6)] = se; red[2 * (t >> 6) + 1] = acc; }
        __syncthreads();
        if (t < 2) {
            const float sum = ((red[t] + red[2 + t]) + red[4 + t]) + red[6 + t];
            a.scratch[(((size_t)n * a.n_cand + cand) * tiles + blockIdx.x) * 2 + t] = sum;
        }
    }
}

// out[k][n] = (psnr, ssim) of candidate k on image n: the image's `tiles` slots added in a fixed order in double
__global__ __launch_bounds__(256) void image_scores_finish_kernel(const float* __restrict__ scratch, int tiles, int n_cand,
                                                                  double count_px, double count_win, float max_val,
                                                                  float* __restrict__ out) {
    __shared__ double sh[2][256];
    const int n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const float* p = scratch + ((size_t)n * n_cand + k) * tiles * 2;
    double se = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) { se += (double)p[2 * (size_t)i]; ss += (double)p[2 * (size_t)i + 1]; }
    sh[0][threadIdx.x] = se; sh[1][threadIdx.x] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* o2 = out + ((size_t)k * N + n) * 2;
        const float mse = (float)(sh[0][0] / count_px);
        o2[0] = 20.0f * log10f(max_val) - 10.0f * log10f(mse);
        o2[1] = (float)(sh[1][0] / count_win);
    }
}

hipError_t launch_image_scores(const ImageScoresArgs& a, int N, float max_val, float* out, hipStream_t s) {
    const int tiles = a.tiles_y * a.tiles_x;
    hipError_t e = launch_with_lds<image_scores_kernel>(dim3(tiles, N), dim3(256), (size_t)scores_lds(a.Ce).bytes, s, a);
    if (e != hipSuccess) return e;
    const double count_px = (double)a.H * (double)a.RL, count_win = (double)(a.H - 10) * (double)(a.RL - 10 * a.Ce);
    hipLaunchKernelGGL(image_scores_finish_kernel, dim3(N, a.n_cand), dim3(256), 0, s, a.scratch, tiles, a.n_cand, count_px,
                       count_win, max_val, out);
    return hipGetLastError();
}

}  // namespace srx
