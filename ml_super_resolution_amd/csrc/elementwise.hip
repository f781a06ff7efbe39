// elementwise.hip -- HBM-bound kernels of the path: sub-pixel index maps, loss, optimizers,
// metrics.  All are grid-stride, 16 B per lane where the layout allows.
#include "elementwise.h"
#include "lds_launch.h"

namespace srx {

// ---------------------------------------------------------------------------------------------
// depth_to_space / space_to_depth.
// For one LR row (n,h) the r HR rows it produces are CONTIGUOUS in the output and cover exactly
// the same flat range [blk*B, (blk+1)*B), B = W*r*r*C, as the LR row does in the input.  So the
// map is one fixed permutation applied independently to every block of B floats:
//   d2s: out[dy*(W*rC) + w*rC + j] = in[w*(r*rC) + dy*rC + j],   rC = r*C
// A workgroup stages RB blocks into LDS with coalesced 16-B loads, gathers from LDS, and writes
// coalesced 16-B stores: HBM traffic is exactly read-once + write-once.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int d2s_src(int oo, int W, int rC, int r, float inv_WrC, float inv_rC) {
    // oo = dy*(W*rC) + w*rC + j  ->  w*(r*rC) + dy*rC + j
    const int WrC = W * rC;
    int dy = (int)(((float)oo + 0.5f) * inv_WrC);
    dy -= (dy * WrC > oo);
    dy += ((dy + 1) * WrC <= oo);
    const int rest = oo - dy * WrC;
    int w = (int)(((float)rest + 0.5f) * inv_rC);
    w -= (w * rC > rest);
    w += ((w + 1) * rC <= rest);
    const int j = rest - w * rC;
    return w * (r * rC) + dy * rC + j;
}

__device__ __forceinline__ int s2d_src(int oo, int W, int rC, int r, float inv_rrC, float inv_rC) {
    // oo = w*(r*rC) + dy*rC + j  ->  dy*(W*rC) + w*rC + j
    const int rrC = r * rC;
    int w = (int)(((float)oo + 0.5f) * inv_rrC);
    w -= (w * rrC > oo);
    w += ((w + 1) * rrC <= oo);
    const int rest = oo - w * rrC;
    int dy = (int)(((float)rest + 0.5f) * inv_rC);
    dy -= (dy * rC > rest);
    dy += ((dy + 1) * rC <= rest);
    const int j = rest - dy * rC;
    return dy * (W * rC) + w * rC + j;
}

// chunk = RB blocks (chunk_floats = RB*B, a multiple of 4).  Every chunk undergoes the SAME
// permutation, so a thread computes the LDS gather indices of its (at most KMAX) output float4s once
// and then only moves data: coalesced 16-B loads -> LDS -> 4 scalar LDS reads -> coalesced 16-B store.
//
// Gather without the 4-way bank conflict of "lane l reads output floats 4l+e in round e" (ds_read_b32 banks
// are (a/4) % 32 per 32-lane half: the lanes of a round sit 4 floats apart and hit 8 banks): in round e lane l
// reads element (e + l/8) % 4 of its float4 instead, so the four 8-lane groups of a half start on banks
// 0,1,2,3 (+ the permutation's own offsets), and the float4 is put back in order with two select stages.
__device__ __forceinline__ f32x4 unrotate4(float a0, float a1, float a2, float a3, bool r1, bool r2) {
    // a_e = element (e + rot) % 4  ->  element j = a_{(j - rot) % 4}: rotate right by rot = r1 + 2 r2
    const float b0 = r1 ? a3 : a0, b1 = r1 ? a0 : a1, b2 = r1 ? a1 : a2, b3 = r1 ? a2 : a3;
    f32x4 o;
    o[0] = r2 ? b2 : b0; o[1] = r2 ? b3 : b1; o[2] = r2 ? b0 : b2; o[3] = r2 ? b1 : b3;
    return o;
}

// The permutation inside a chunk as index arithmetic.  With (N1, N2) = (r, W) for depth-to-space and (W, r) for its
// inverse, an output position and its source are
//   o   = blk*B + a*(N2*rC) + b*rC + j,      a < N1, b < N2, j < rC,  B = N1*N2*rC
//   src = blk*B + b*(N1*rC) + a*rC + j
// (the two inner digits swap places).  Divisions are multiplications by host-computed reciprocals
// M = floor(2^32 / d) + 1 (exact for o * d < 2^32: o < 2^14 floats of LDS, d <= B < 2^14), every product fits 24 bits.
struct SubpixelGeom {
    int B, N1, N2, rC;          // block length, outer / inner digit ranges, run length
    unsigned mA, mR, m1;        // reciprocals of N2*rC, rC, N1
};

inline SubpixelGeom subpixel_geom(int W, int rC, int r, bool inverse) {
    SubpixelGeom g;
    g.N1 = inverse ? W : r;
    g.N2 = inverse ? r : W;
    g.rC = rC;
    g.B = W * r * rC;
    auto magic = [](unsigned d) { return (unsigned)((1ull << 32) / d) + 1u; };   // (d = 1 is handled by the caller)
    g.mA = magic((unsigned)(g.N2 * rC));
    g.mR = magic((unsigned)rC);
    g.m1 = magic((unsigned)g.N1);
    return g;
}

struct SubpixelIndex {
    SubpixelGeom g;
    __device__ explicit SubpixelIndex(const SubpixelGeom& g_) : g(g_) {}
    static __device__ __forceinline__ int divq(int o, int d, unsigned m) { return d == 1 ? o : (int)__umulhi((unsigned)o, m); }
    // digits of position o
    __device__ __forceinline__ void digits(int o, int& blk, int& a, int& b, int& j) const {
        const int A = g.N2 * g.rC;
        const int R = divq(o, A, g.mA);              // R = blk*N1 + a
        const int rest = o - __mul24(R, A);
        b = divq(rest, g.rC, g.mR);
        j = rest - __mul24(b, g.rC);
        blk = divq(R, g.N1, g.m1);
        a = R - __mul24(blk, g.N1);
    }
    __device__ __forceinline__ int src(int blk, int a, int b, int j) const {
        return __mul24(blk, g.B) + __mul24(b, __mul24(g.N1, g.rC)) + __mul24(a, g.rC) + j;
    }
    __device__ __forceinline__ int operator()(int o) const {
        int blk, a, b, j;
        digits(o, blk, a, b, j);
        return src(blk, a, b, j);
    }
    // sources of the four consecutive positions o .. o+3: one digit decomposition, then
    //  * runs of at least 4 (rC >= 4: every case of the reference, rC = 3r): at most ONE digit wrap inside the four, at
    //    element rC - j; before it the source advances by 1 per element, from it on by 1 per element plus one jump whose
    //    size depends on how far the carry goes (b, a, block);
    //  * shorter runs: odometer steps.
    __device__ __forceinline__ void four(int o, int (&out)[4]) const {
        int blk, a, b, j;
        digits(o, blk, a, b, j);
        const int s0 = src(blk, a, b, j);
        out[0] = s0;
        // source increments when a digit wraps: j wraps -> b+1; b wraps -> a+1; a wraps -> blk+1
        const int N1rC = __mul24(g.N1, g.rC);
        const int dj = N1rC - (g.rC - 1);                                // (b+1, 0) - (b, rC-1)
        const int db = g.rC - __mul24(g.N2 - 1, N1rC) - (g.rC - 1);        // (a+1, 0, 0) - (a, N2-1, rC-1)
        const int da = g.B - __mul24(g.N1 - 1, g.rC) - __mul24(g.N2 - 1, N1rC) - (g.rC - 1);   // next block's first
        if (g.rC >= 4) {   // (wave-uniform)
            const bool wb = b == g.N2 - 1, wa = wb && a == g.N1 - 1;
            const int jump = (wa ? da : (wb ? db : dj)) - 1;
            const int at = g.rC - j;                                     // first element behind the wrap (>= 1)
#pragma unroll
            for (int e = 1; e < 4; ++e) out[e] = s0 + e + (e >= at ? jump : 0);
            return;
        }
        int s = s0;
#pragma unroll
        for (int e = 1; e < 4; ++e) {
            ++j;
            const bool wj = j == g.rC;
            j = wj ? 0 : j;
            b += wj;
            const bool wb = b == g.N2;
            b = wb ? 0 : b;
            a += wb;
            const bool wa = a == g.N1;
            a = wa ? 0 : a;
            s += wa ? da : (wb ? db : (wj ? dj : 1));
            out[e] = s;
        }
    }
    // the four sources of float4 slot i of a chunk of c4 float4s, in the rotated order of the gather: entry e is the
    // source of element (e + rot) % 4; slots beyond the chunk get 0
    // the same for four consecutive positions o0 .. o0+3 that need not start a float4 of the chunk (subpixel_even_kernel:
    // the output side is aligned to the 128-byte lines of global memory, not to the chunk); ok = all four inside the chunk
    __device__ __forceinline__ void rotated_at(int o0, bool ok, int rot, int (&out)[4]) const {
        int t[4];
        four(ok ? o0 : 0, t);
        const bool r1 = rot & 1, r2 = rot & 2;
        const int u0 = r1 ? t[1] : t[0], u1 = r1 ? t[2] : t[1], u2 = r1 ? t[3] : t[2], u3 = r1 ? t[0] : t[3];
        out[0] = ok ? (r2 ? u2 : u0) : 0;
        out[1] = ok ? (r2 ? u3 : u1) : 0;
        out[2] = ok ? (r2 ? u0 : u2) : 0;
        out[3] = ok ? (r2 ? u1 : u3) : 0;
    }
    __device__ __forceinline__ void rotated(int i, int c4, int rot, int (&out)[4]) const {
        int t[4];
        four(4 * i, t);
        const bool r1 = rot & 1, r2 = rot & 2, in = i >= 0 && i < c4;
        // entry e = t[(e + rot) % 4]: rotate left by rot
        const int u0 = r1 ? t[1] : t[0], u1 = r1 ? t[2] : t[1], u2 = r1 ? t[3] : t[2], u3 = r1 ? t[0] : t[3];
        out[0] = in ? (r2 ? u2 : u0) : 0;
        out[1] = in ? (r2 ? u3 : u1) : 0;
        out[2] = in ? (r2 ? u0 : u2) : 0;
        out[3] = in ? (r2 ? u1 : u3) : 0;
    }
};

// One LDS buffer, any chunk length (the last chunk of a tensor may be short and need not be a multiple of 4 floats):
// rows too long for two buffers, and the ragged tail behind the pipelined kernel below.
template <int KMAX>
__global__ __launch_bounds__(256) void subpixel_lds_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           size_t total, int chunk_floats, SubpixelGeom geo) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SubpixelIndex src_of(geo);
    const int c4 = chunk_floats >> 2;
    const int rot = (threadIdx.x >> 3) & 3;
    const bool r1 = rot & 1, r2 = rot & 2;
    int sidx[KMAX][4];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) src_of.rotated(k * 256 + threadIdx.x, c4, rot, sidx[k]);
    for (size_t c0 = (size_t)blockIdx.x * chunk_floats; c0 < total; c0 += (size_t)gridDim.x * chunk_floats) {
        const int n = (int)((total - c0 < (size_t)chunk_floats) ? (total - c0) : (size_t)chunk_floats);
        const int n4 = n >> 2;
        const f32x4* gin = reinterpret_cast<const f32x4*>(in + c0);
        f32x4* gout = reinterpret_cast<f32x4*>(out + c0);
        f32x4 v[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int i = k * 256 + threadIdx.x;
            if (i < n4) v[k] = __builtin_nontemporal_load(gin + i);   // streamed once: keep it out of L2
        }
        __syncthreads();   // previous chunk's gathers are done
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int i = k * 256 + threadIdx.x;
            if (i < n4) reinterpret_cast<f32x4*>(lds)[i] = v[k];
        }
        for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) lds[i] = in[c0 + i];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int i = k * 256 + threadIdx.x;
            if (i < n4)
                __builtin_nontemporal_store(unrotate4(lds[sidx[k][0]], lds[sidx[k][1]], lds[sidx[k][2]], lds[sidx[k][3]], r1, r2),
                                            gout + i);
        }
        for (int o = (n4 << 2) + threadIdx.x; o < n; o += 256) out[c0 + o] = lds[src_of(o)];
    }
}

// The same map over FULL chunks (chunk_floats each; the launcher sends a ragged tail to the kernel above) with the next
// chunk's loads in flight, held in registers, while the workgroup gathers the current one.
// What bounds a 93-MB transfer is how many of its bytes are in flight from the first microsecond on
// (scripts/d2s_ubench.hip: a plain copy with 8 float4 per thread on 2048 workgroups -- every load of the tensor issued at
// once -- takes 15.3 us; the same copy in two rounds of 4 float4 per thread 17.4 us; this kernel's chunk structure with
// one chunk of loads per workgroup in flight and NO gather at all 18.0 us).  Requesting all of a workgroup's 2-3 chunks
// before touching the first one was measured slower.
// * Two LDS buffers, one barrier per chunk (a thread that writes buffer p for chunk c has passed the barrier of chunk
//   c-1, which every thread reaches only after its gather of chunk c-2 from the same buffer).
// * No predicated memory instruction and no branch in a trip: loads and stores are bounds-checked buffer operations (a
//   float4 past the end of the chunk reads zeros / is dropped; a chunk at or beyond nfull has an EMPTY resource, so the
//   last trip's loads of the next chunk read zeros and touch no memory), LDS writes of lanes beyond the chunk go to a
//   per-thread dummy slot.  With every access unconditional the compiler's waits are COUNTED
//   (s_waitcnt vmcnt(n)): an LDS write waits for its own chunk's loads only, not for younger loads and stores.
//   (Per-lane `if (i < n4)` around each access makes them vmcnt(0).)  The dropped stores of the prologue put the
//   vector-memory queue into the state every later trip finds at the loop top, so that the counts are the steady-state
//   ones instead of the minimum over the two ways into the loop.
// * The loads go out before the index computation, which then runs under the memory latency.
// * The barrier is the raw s_barrier behind an LDS-only wait: __syncthreads() would also drain the vector-memory queue.
// KMAX = ceil(chunk_floats / 4 / 256): only the last slot has lanes beyond the chunk.
// At most 3 vector-memory requests of a wave in flight (s_waitcnt vmcnt(2) behind every load and store).
// More is NOT better for a streaming kernel on this memory system (scripts/d2s_ubench.hip, profiles/r03_d2s_ubench.txt):
// the fastest plain copy of this tensor keeps ONE request per wave in flight at 32 waves per CU (15.5 us); the same copy
// with 6 per wave takes 17.3 us.  At this kernel's 16 waves per CU (a copy in its structure): 1 -> 19.1, 2 -> 17.0, 3 -> 16.6,
// 4 -> 16.0, unbounded (the 5 loads of the next chunk + the 5 stores of this one) 16.9 us; the kernel itself: unbounded 17.5,
// 2 -> 17.1, 3 -> 16.8, 4 -> 17.0, 5-8 -> 17.2 us.
template <int KMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))   // four workgroups per CU: <= 128 registers
void subpixel_pipe_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int nfull, int chunk_floats, SubpixelGeom geo) {
    constexpr int DEPTH = 1;   // chunks of loads in flight per workgroup (deeper: measured slower)
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [2][chunk_floats] + [256][4] dummy slots
    int c = blockIdx.x;
    if (c >= nfull) return;
    const int G = gridDim.x;
    const int c4 = chunk_floats >> 2;
    const unsigned chunk_bytes = (unsigned)chunk_floats * 4u;
    const int lane_off = threadIdx.x * 16;
    auto rsrc_at = [&](const float* base, int chunk) {
        const bool ok = chunk < nfull;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (size_t)(ok ? chunk : 0) * chunk_floats), 0,
                                                 ok ? chunk_bytes : 0u, 0x00020000);
    };
    auto throttle = [&]() { asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); };
    u32x4v v[DEPTH][KMAX];
    // (the first chunk's loads are not throttled: the wave goes on to its index arithmetic, not to more requests)
    auto issue = [&](u32x4v (&dst)[KMAX], int chunk, bool throttled) {
        const __amdgpu_buffer_rsrc_t rs = rsrc_at(in, chunk);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            dst[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off + k * 4096, 0, 2 /* nt */);
            if (throttled) throttle();
        }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        issue(v[d], c + d * G, false);
        const __amdgpu_buffer_rsrc_t rs = rsrc_at(out, nfull);   // empty: the stores are dropped
        const u32x4v z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < KMAX; ++k) __builtin_amdgcn_raw_buffer_store_b128(z, rs, lane_off + k * 4096, 0, 2);
    }
    const SubpixelIndex src_of(geo);
    const int rot = (threadIdx.x >> 3) & 3;
    const bool r1 = rot & 1, r2 = rot & 2;
    // STORES IN WHOLE 128-BYTE LINES.  A chunk is a whole number of blocks, not of cache lines (17,712 bytes at
    // [.,41,41,27]: chunk c starts 48 c mod 128 bytes into a line), and a wave's store instruction that starts inside a
    // line leaves two partial lines behind.  That alone costs a plain copy of this tensor 12 % (scripts/d2s_ubench.hip:
    // 15.6 us with the destination on a line boundary, 17.5 us 48 bytes off it; the source's alignment is free).  So the
    // lane <-> float4 assignment of the OUTPUT side is shifted down by `shift` float4s: lane i gathers and stores the
    // chunk's float4 i - shift, which makes every store instruction start on a line boundary (only the chunk's first
    // and last line are shared with the neighbouring chunks).  All chunks of a workgroup start at the same offset
    // into a line (the launcher makes the grid a multiple of the period, at most 8), so the shift -- and with it the
    // gather table -- is fixed per workgroup.  Lanes left of the chunk get a negative buffer offset: out of range as
    // an unsigned number, the store is dropped.
    const int shift = (int)((reinterpret_cast<uintptr_t>(out) + (size_t)c * chunk_bytes) & 127u) >> 4;
    // gather sources as LDS byte offsets inside a buffer, two per register (a buffer is < 64 KB): the DEPTH chunks of
    // data in flight need the registers
    unsigned spk[KMAX][2];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        int t[4];
        src_of.rotated(k * 256 + threadIdx.x - shift, c4, rot, t);
        spk[k][0] = (unsigned)(t[0] * 4) | ((unsigned)(t[1] * 4) << 16);
        spk[k][1] = (unsigned)(t[2] * 4) | ((unsigned)(t[3] * 4) << 16);
    }
    const int store_off = lane_off - 16 * shift;
    // LDS float4 slots of the last TWO load slots: inside the chunk, or this thread's dummy slot.  KMAX counts STORE
    // slots, i.e. it includes the up-to-7-float4 shift: c4 > 256 (KMAX - 1) - 7 only, so when c4 % 256 is 250..255 the
    // slot before the last also has lanes past the chunk -- written unguarded they would land in the first float4s of
    // the OTHER buffer, which slower waves may still be gathering from (round-3 advisor finding; every slot below
    // KMAX - 2 lies inside the chunk: 256 (KMAX - 2) <= c4).
    const int last_i = (KMAX - 1) * 256 + threadIdx.x;
    const bool last_in = last_i < c4;
    const int prev_i = (KMAX >= 2 ? KMAX - 2 : 0) * 256 + threadIdx.x;
    const bool prev_in = prev_i < c4;
    auto step = [&](u32x4v (&reg)[KMAX], int p, int cur) {
        float* buf = lds + p * chunk_floats;
        u32x4v* buf4 = reinterpret_cast<u32x4v*>(buf);
#pragma unroll
        for (int k = 0; k < KMAX - 2; ++k) buf4[k * 256 + threadIdx.x] = reg[k];
        if constexpr (KMAX >= 2)
            reinterpret_cast<u32x4v*>(lds)[prev_in ? p * c4 + prev_i : 2 * c4 + threadIdx.x] = reg[KMAX - 2];
        reinterpret_cast<u32x4v*>(lds)[last_in ? p * c4 + last_i : 2 * c4 + threadIdx.x] = reg[KMAX - 1];
        issue(reg, cur + DEPTH * G, true);
        lds_barrier();
        const __amdgpu_buffer_rsrc_t ro = rsrc_at(out, cur);
        const char* bytes = reinterpret_cast<const char*>(buf);
        constexpr int GB = 3;   // float4s gathered per batch: their LDS reads are issued together (one latency per batch)
#pragma unroll
        for (int k0 = 0; k0 < KMAX; k0 += GB) {
            float g[GB][4];
#pragma unroll
            for (int k = k0; k < k0 + GB && k < KMAX; ++k) {
                g[k - k0][0] = *reinterpret_cast<const float*>(bytes + (spk[k][0] & 0xffffu));
                g[k - k0][1] = *reinterpret_cast<const float*>(bytes + (spk[k][0] >> 16));
                g[k - k0][2] = *reinterpret_cast<const float*>(bytes + (spk[k][1] & 0xffffu));
                g[k - k0][3] = *reinterpret_cast<const float*>(bytes + (spk[k][1] >> 16));
            }
#pragma unroll
            for (int k = k0; k < k0 + GB && k < KMAX; ++k) {
                const f32x4 o = unrotate4(g[k - k0][0], g[k - k0][1], g[k - k0][2], g[k - k0][3], r1, r2);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, o), ro, store_off + k * 4096, 0, 2);
                throttle();
            }
        }
    };
    for (int n = 0; c < nfull; c += DEPTH * G, n += DEPTH) {   // n: chunks this workgroup has done (LDS buffer = parity)
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) step(v[d], (n + d) & 1, c + d * G);
    }
}

// EVEN chunks.  subpixel_pipe_kernel's chunks are whole multiples of 4 blocks (so that every chunk starts a float4):
// 2,624 chunks of 17.7 KB at [256,41,41,27], i.e. three trips for 576 of the 1,024 persistent workgroups and two for the
// rest, and two LDS buffers of 17.7 KB are all that fits four workgroups per CU.  What a streaming kernel of this shape
// pays for is the number of TRIPS (scripts/d2s_direct_ubench.hip: the pipe kernel's structure as a copy 16.2 us, three
// equal trips of 15 KB 16.8 us, four of 11 KB 17.8 us -- and TWO trips of 22.6 KB for every workgroup 15.3 us, below
// the plain one-round copy).  Here a chunk is ANY whole number of blocks: the tensor's `nblocks` blocks are dealt out
// as `nchunks` = trips * grid chunks of q or q+1 blocks, chunk c -> workgroup c % grid.
//  * A chunk starts at any 4-byte offset: its 16-byte loads go out from there (source alignment is free: 15.5 us
//    either way, same benchmark) and the chunk sits at offset 0 of ONE LDS buffer (a chunk of up to 32 KB; the next chunk's
//    loads wait in registers, as before).
//  * The output side is aligned to the 128-byte lines of global memory instead: float4 slot j of a workgroup is the
//    16 bytes at line_base + 16 j, i.e. positions 4 j - sf .. + 3 of the chunk (sf = floats between the line boundary below
//    the chunk and the chunk, < 32).  Slots entirely inside the chunk are gathered and stored as before; the at most
//    two float4s a chunk shares with its neighbours are written float by float by one lane each.
//  * sf and the chunk length differ from chunk to chunk, so the gather table is computed per chunk -- between issuing
//    the chunk's loads and the gather of the chunk before it, i.e. under the loads' latency.
template <int KMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))   // four workgroups per CU: <= 128 registers
void subpixel_even_kernel(const float* __restrict__ in, float* __restrict__ out, size_t total, int nchunks, int q, int rem,
                          int lds_floats, SubpixelGeom geo) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [lds_floats] + [256][4] dummy slots
    const int G = gridDim.x;
    const int tid = threadIdx.x;
    const int lane_off = tid * 16;
    const SubpixelIndex src_of(geo);
    const int rot = (tid >> 3) & 3;
    const bool r1 = rot & 1, r2 = rot & 2;
    // at most 2 vector-memory requests of a wave in flight (see launch_subpixel)
    auto throttle = [&]() { asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); };
    struct Chunk { size_t S; int L, sf; };   // first float, floats, floats between the 128-byte line below out + S and out + S
    auto chunk_of = [&](int c) {
        Chunk k;
        const int b0 = c * q + (c < rem ? c : rem);                    // the first `rem` chunks have q + 1 blocks
        k.S = (size_t)b0 * (size_t)geo.B;
        k.L = (q + (c < rem ? 1 : 0)) * geo.B;
        k.sf = (int)((reinterpret_cast<uintptr_t>(out + k.S) & 127u) >> 2);
        return k;
    };
    u32x4v v[KMAX];
    // whole float4s from the chunk's first float on; the last one may reach up to 3 floats into the next chunk, except at
    // the end of the tensor: there the ragged floats are fetched one by one (to_lds)
    auto whole4 = [&](const Chunk& ch) { const int up = (ch.L + 3) & ~3; return ch.S + (size_t)up <= total ? up : (ch.L & ~3); };
    auto issue = [&](const Chunk& ch, bool throttled) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in + ch.S), 0, (unsigned)whole4(ch) * 4u, 0x00020000);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off + k * 4096, 0, 2 /* nt */);
            if (throttled) throttle();
        }
    };
    auto to_lds = [&](const Chunk& ch) {
        const int w4 = whole4(ch), n4 = w4 >> 2, dummy = (lds_floats >> 2) + tid;
        u32x4v* buf4 = reinterpret_cast<u32x4v*>(lds);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { const int j = k * 256 + tid; buf4[j < n4 ? j : dummy] = v[k]; }
        if (w4 < ch.L && tid < ch.L - w4) lds[w4 + tid] = in[ch.S + w4 + tid];      // (the tensor's last chunk only)
    };
    auto table = [&](const Chunk& ch, unsigned (&spk)[KMAX][2]) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int o0 = 4 * (k * 256 + tid) - ch.sf;
            int t[4];
            src_of.rotated_at(o0, o0 >= 0 && o0 + 4 <= ch.L, rot, t);
            spk[k][0] = (unsigned)(t[0] * 4) | ((unsigned)(t[1] * 4) << 16);
            spk[k][1] = (unsigned)(t[2] * 4) | ((unsigned)(t[3] * 4) << 16);
        }
    };
    auto drain = [&](const Chunk& ch, const unsigned (&spk)[KMAX][2]) {
        float* line = out + ch.S - ch.sf;                                  // (128-byte aligned)
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(line, 0, (unsigned)(ch.sf + ch.L) * 4u, 0x00020000);
        const char* bytes = reinterpret_cast<const char*>(lds);
        constexpr int GB = 3;   // float4s gathered per batch: their LDS reads are issued together (one latency per batch)
#pragma unroll
        for (int k0 = 0; k0 < KMAX; k0 += GB) {
            float g[GB][4];
#pragma unroll
            for (int k = k0; k < k0 + GB && k < KMAX; ++k) {
                g[k - k0][0] = *reinterpret_cast<const float*>(bytes + (spk[k][0] & 0xffffu));
                g[k - k0][1] = *reinterpret_cast<const float*>(bytes + (spk[k][0] >> 16));
                g[k - k0][2] = *reinterpret_cast<const float*>(bytes + (spk[k][1] & 0xffffu));
                g[k - k0][3] = *reinterpret_cast<const float*>(bytes + (spk[k][1] >> 16));
            }
#pragma unroll
            for (int k = k0; k < k0 + GB && k < KMAX; ++k) {
                const f32x4 o = unrotate4(g[k - k0][0], g[k - k0][1], g[k - k0][2], g[k - k0][3], r1, r2);
                const int j = k * 256 + tid, o0 = 4 * j - ch.sf;
                // a float4 not entirely inside the chunk: an offset past the resource, the store is dropped
                const unsigned off = (o0 >= 0 && o0 + 4 <= ch.L) ? (unsigned)j * 16u : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, o), ro, off, 0, 2);
                throttle();
            }
        }
        // the float4s shared with the neighbouring chunks: one lane each, float by float
        const int jh = ch.sf >> 2, jt = (ch.sf + ch.L) >> 2;
        if ((tid == 0 && (ch.sf & 3)) || (tid == 64 && ((ch.sf + ch.L) & 3))) {
            const int o0 = 4 * (tid == 0 ? jh : jt) - ch.sf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = o0 + e;
                if (o >= 0 && o < ch.L) out[ch.S + o] = lds[src_of(o)];
            }
        }
    };
    int c = blockIdx.x;
    if (c >= nchunks) return;
    Chunk cur = chunk_of(c), nxt = cur;
    // (the first chunk's loads are not throttled -- the wave goes on to its index arithmetic, not to more requests;
    // throttled and interleaved with the arithmetic: 17.2 instead of 16.4 us)
    issue(cur, false);
    unsigned tab[KMAX][2], tab_n[KMAX][2];
    table(cur, tab);
    for (;;) {
        lds_barrier();                       // every wave is done gathering the chunk before
        to_lds(cur);
        const bool more = c + G < nchunks;
        if (more) {
            nxt = chunk_of(c + G);
            // (chunks G apart often have the same length and the same offset into a line: the table carries over)
            issue(nxt, true);      // (unthrottled: 17.2 instead of 16.4 us)
            if (nxt.L != cur.L || nxt.sf != cur.sf) {
                table(nxt, tab_n);
            } else {
#pragma unroll
                for (int k = 0; k < KMAX; ++k) { tab_n[k][0] = tab[k][0]; tab_n[k][1] = tab[k][1]; }
            }
        }
        lds_barrier();
        drain(cur, tab);
        if (!more) break;
        c += G; cur = nxt;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { tab[k][0] = tab_n[k][0]; tab[k][1] = tab_n[k][1]; }
    }
}

// What a plain streaming copy of the same bytes reaches with the same launch shape (persistent workgroups, KMAX
// nontemporal 16-B loads in flight per thread, nontemporal stores): the ceiling the sub-pixel map is measured
// against (bench.py `subpixel.copy_ceiling_gbps`).
template <int KMAX>
__global__ __launch_bounds__(256) void stream_copy_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, size_t n4) {
    const size_t per = (size_t)KMAX * 256;
    for (size_t base = (size_t)blockIdx.x * per; base < n4; base += (size_t)gridDim.x * per) {
        f32x4 v[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const size_t i = base + (size_t)k * 256 + threadIdx.x;
            if (i < n4) v[k] = __builtin_nontemporal_load(in + i);
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const size_t i = base + (size_t)k * 256 + threadIdx.x;
            if (i < n4) __builtin_nontemporal_store(v[k], out + i);
        }
    }
}

hipError_t launch_stream_copy(const float* in, float* out, size_t bytes, hipStream_t s) {
    const size_t n4 = bytes / 16;
    if (n4 == 0) return hipSuccess;
    const size_t per = 8 * 256;
    size_t nb = (n4 + per - 1) / per;
    const int grid = (int)(nb < 2048 ? nb : 2048);
    hipLaunchKernelGGL(stream_copy_kernel<8>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const f32x4*>(in),
                       reinterpret_cast<f32x4*>(out), n4);
    return hipGetLastError();
}

// Fallback for rows too long for LDS: direct gather (reads stay inside one B-float block).
template <bool INVERSE>
__global__ __launch_bounds__(256) void subpixel_direct_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              size_t total, int B, int W, int rC, int r) {
    const float inv_a = INVERSE ? 1.0f / (float)(r * rC) : 1.0f / (float)(W * rC);
    const float inv_rC = 1.0f / (float)rC;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const size_t blk = o / (size_t)B;
        const int oo = (int)(o - blk * (size_t)B);
        const int src = INVERSE ? s2d_src(oo, W, rC, r, inv_a, inv_rC) : d2s_src(oo, W, rC, r, inv_a, inv_rC);
        out[o] = in[blk * (size_t)B + src];
    }
}

hipError_t launch_subpixel(const float* in, float* out, int N, int H, int W, int C, int r, bool inverse, int max_grid,
                           hipStream_t s) {
    const int rC = r * C;
    const size_t B = (size_t)W * r * rC;
    const size_t total = (size_t)N * H * B;
    if (total == 0) return hipSuccess;
    const size_t lds_cap = 48 * 1024;
    // RB blocks per chunk: chunk must be a multiple of 4 floats so every chunk start is 16-B aligned
    size_t RB = 4;
    if (B % 4 == 0) RB = 1; else if (B % 2 == 0) RB = 2;
    // even chunks of whole blocks (subpixel_even_kernel): a tensor of whole float4s with at least a few blocks per CU
    // whose block fits 8 float4 slots per thread beside the output side's shift
    constexpr size_t kEvenMaxFloats = 8 * 1024 - 34;
    const size_t nblocks = (size_t)N * H;
    size_t even_trips = 0, even_grid = 0;
    if (total % 4 == 0 && nblocks >= 512 && nblocks < (1u << 30) && B <= kEvenMaxFloats) {
        even_grid = nblocks < (size_t)max_grid ? nblocks : (size_t)max_grid;
        even_trips = 1;
        auto max_blocks = [&](size_t t) { return (nblocks + even_grid * t - 1) / (even_grid * t); };
        while (max_blocks(even_trips) > 1 && max_blocks(even_trips) * B > kEvenMaxFloats) ++even_trips;
        // One LDS buffer: its barrier phases are not hidden behind a second buffer's traffic.  Up to two trips per
        // workgroup that is the better trade (16.5 against 16.9 us at [256,41,41,27], 18.3 against 19.6 at [128,64,64,27]);
        // from three trips on subpixel_pipe_kernel's two buffers win (28.1 against 27.6 us at [256,41,41,48], 69.5 against
        // 62.5 at [1024,41,41,27]: scripts/time_d2s.py shapes).
        if (even_trips > 2) even_trips = 0;
    }
    if (even_trips) {
        const SubpixelGeom geo = subpixel_geom(W, rC, r, inverse);
        const size_t grid = even_grid, trips = even_trips;
        const size_t nchunks = grid * trips < nblocks ? grid * trips : nblocks;
        const int q = (int)(nblocks / nchunks), rem = (int)(nblocks % nchunks);
        const size_t lmax = (size_t)(q + (rem ? 1 : 0)) * B;
        const int lds_floats = (int)((lmax + 3) & ~(size_t)3);
        const size_t lds_bytes = (size_t)lds_floats * 4 + 4096;
        const int kneed = (int)(((lmax + 31 + 3) / 4 + 255) / 256);
        // (measured at [256,41,41,27], alternating runs on three boxes: 16.4-16.6 us with 2 requests per wave in flight, 16.8-17.2
        // with 3; subpixel_pipe_kernel -- three trips of smaller chunks for half of the workgroups -- has its optimum at 3.
        // Eight waves per workgroup with one request each: 16.5-16.8.)
#define SRX_SUBPIXEL_EVEN(K) case K: hipLaunchKernelGGL((subpixel_even_kernel<K>), dim3((unsigned)grid), dim3(256), lds_bytes, s, in, out, total, (int)nchunks, q, rem, lds_floats, geo); break;
        switch (kneed) {
            SRX_SUBPIXEL_EVEN(1) SRX_SUBPIXEL_EVEN(2) SRX_SUBPIXEL_EVEN(3) SRX_SUBPIXEL_EVEN(4)
            SRX_SUBPIXEL_EVEN(5) SRX_SUBPIXEL_EVEN(6) SRX_SUBPIXEL_EVEN(7) SRX_SUBPIXEL_EVEN(8)
            default: return hipErrorInvalidValue;
        }
#undef SRX_SUBPIXEL_EVEN
        return hipGetLastError();
    }
    if (RB * B * 4 <= lds_cap && B < (1u << 20)) {
        const SubpixelGeom geo = subpixel_geom(W, rC, r, inverse);
        while (2 * RB * B * 4 <= 24 * 1024) RB *= 2;   // ~16-24 KiB chunks: several workgroups per CU
        const int chunk = (int)(RB * B);
        const size_t nchunks = (total + chunk - 1) / chunk;
        const size_t cap = (size_t)max_grid;   // persistent workgroups: the index precomputation is paid once each
        const int kneed = (chunk / 4 + 7 + 255) / 256;   // (+7: the pipelined kernel's output side is shifted by up to 7 float4s)
        // the software-pipelined kernel: two LDS buffers + the dummy slots while four workgroups still share a CU
        const size_t pipe_lds = (size_t)chunk * 8 + 4096;
        const size_t nfull = pipe_lds <= 40 * 1024 && kneed <= 8 && nchunks < (1u << 28) ? total / chunk : 0;
        if (nfull) {
            int grid = (int)(nfull < cap ? nfull : cap);
            if ((size_t)grid < nfull && grid >= 8) grid -= grid % 8;   // every chunk of a workgroup starts at the same offset into a 128-byte line (a cap below 8 keeps its grid: the shift is computed from the first chunk and only costs alignment)
#define SRX_SUBPIXEL_PIPE(K) case K: hipLaunchKernelGGL((subpixel_pipe_kernel<K>), dim3(grid), dim3(256), pipe_lds, s, in, out, (int)nfull, chunk, geo); break;
            switch (kneed) {
                SRX_SUBPIXEL_PIPE(1) SRX_SUBPIXEL_PIPE(2) SRX_SUBPIXEL_PIPE(3) SRX_SUBPIXEL_PIPE(4)
                SRX_SUBPIXEL_PIPE(5) SRX_SUBPIXEL_PIPE(6) SRX_SUBPIXEL_PIPE(7) SRX_SUBPIXEL_PIPE(8)
            }
#undef SRX_SUBPIXEL_PIPE
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        const size_t done = nfull * (size_t)chunk;
        if (done < total) {   // everything (single-buffer route) or the ragged last chunk
            const float* tin = in + done;
            float* tout = out + done;
            const size_t ttotal = total - done;
            const size_t tchunks = (ttotal + chunk - 1) / chunk;
            const int grid = (int)(tchunks < cap ? tchunks : cap);
#define SRX_SUBPIXEL_LAUNCH(K)                                                                                   \
            hipLaunchKernelGGL((subpixel_lds_kernel<K>), dim3(grid), dim3(256), chunk * 4, s, tin, tout, ttotal, chunk, geo);
            const int kplain = (chunk / 4 + 255) / 256;     // (no shift here: float4 slots of the chunk itself, <= 12 for 48 KiB)
            if (kplain <= 4) { SRX_SUBPIXEL_LAUNCH(4) }
            else if (kplain <= 8) { SRX_SUBPIXEL_LAUNCH(8) }
            else { SRX_SUBPIXEL_LAUNCH(12) }
#undef SRX_SUBPIXEL_LAUNCH
        }
    } else {
        if (B >= (1u << 22)) return hipErrorInvalidValue;
        size_t nb = (total + 255) / 256;
        int grid = (int)(nb < 8192 ? nb : 8192);
        if (inverse)
            hipLaunchKernelGGL(subpixel_direct_kernel<true>, dim3(grid), dim3(256), 0, s, in, out, total, (int)B, W, rC, r);
        else
            hipLaunchKernelGGL(subpixel_direct_kernel<false>, dim3(grid), dim3(256), 0, s, in, out, total, (int)B, W, rC, r);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// reductions: per-block partials (fixed grid) -> one finishing block, double accumulate.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float t = (threadIdx.x < (blockDim.x >> 6)) ? sh[threadIdx.x] : 0.f;
    if (wave == 0) t = wave_sum(t);
    return t;  // valid in wave 0
}

// MODE 0: (a-b)^2, also writes dpred = 2*(a-b)*inv ; MODE 1: a^2 (times b as a 0/1 mask when b != null)
template <int MODE>
__global__ __launch_bounds__(256) void sq_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         size_t n, float inv, float* __restrict__ dpred,
                                                         float* __restrict__ partial) {
    __shared__ float sh[4];
    float acc = 0.f;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 va = reinterpret_cast<const f32x4*>(a)[i];
        if (MODE == 0) {
            const f32x4 vb = reinterpret_cast<const f32x4*>(b)[i];
            va -= vb;
            if (dpred) reinterpret_cast<f32x4*>(dpred)[i] = va * (2.0f * inv);
            acc += va[0] * va[0] + va[1] * va[1] + va[2] * va[2] + va[3] * va[3];
        } else if (b) {
            const f32x4 m = reinterpret_cast<const f32x4*>(b)[i];
            acc += m[0] * va[0] * va[0] + m[1] * va[1] * va[1] + m[2] * va[2] * va[2] + m[3] * va[3] * va[3];
        } else {
            acc += va[0] * va[0] + va[1] * va[1] + va[2] * va[2] + va[3] * va[3];
        }
    }
    if (blockIdx.x == 0) {
        for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            float d = a[i];
            if (MODE == 0) {
                d -= b[i];
                if (dpred) dpred[i] = d * (2.0f * inv);
            }
            acc += (MODE == 1 && b) ? b[i] * d * d : d * d;
        }
    }
    const float t = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void finish_sum_kernel(const float* __restrict__ partial, int n, float scale,
                                                         float* __restrict__ out, int accumulate) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float v = (float)(sh[0] * (double)scale);
        out[0] = accumulate ? out[0] + v : v;
    }
}

static int reduce_grid(size_t n) {
    size_t nb = ((n >> 2) + 255) / 256;
    if (nb < 1) nb = 1;
    return (int)(nb < (size_t)kReduceBlocks ? nb : (size_t)kReduceBlocks);
}

hipError_t launch_mse(const float* pred, const float* target, size_t n, float inv, float* loss, int accumulate,
                      float* dpred, float* scratch, hipStream_t s) {
    const int grid = reduce_grid(n);
    hipLaunchKernelGGL(sq_partial_kernel<0>, dim3(grid), dim3(256), 0, s, pred, target, n, inv, dpred, scratch);
    if (loss) hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, s, scratch, grid, inv, loss, accumulate);
    return hipGetLastError();
}

hipError_t launch_l2(const float* w, const float* mask, size_t n, float scale, float* loss, int accumulate,
                     float* scratch, hipStream_t s) {
    const int grid = reduce_grid(n);
    hipLaunchKernelGGL(sq_partial_kernel<1>, dim3(grid), dim3(256), 0, s, w, mask, n, 0.f,
                       (float*)nullptr, scratch);
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, s, scratch, grid, 0.5f * scale, loss, accumulate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// optimizers (flat buffers)
// ---------------------------------------------------------------------------------------------
// One element of the update, shared by both Adam kernels below so that they round identically (left to the compiler, the
// two kernels contracted `b1 * m + ob1 * g` into different fused multiply-adds: slots one ulp apart whenever b1 * m is inexact
// -- found by scripts/fuzz_round4.py).  m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2, the smaller product rounded first.
__device__ __forceinline__ void adam_elem(float& w, float g, float& m, float& v, float lr_t, float b1, float b2, float ob1,
                                          float ob2, float eps) {
    m = fmaf(b1, m, ob1 * g);
    v = fmaf(b2, v, ob2 * (g * g));
    w -= lr_t * m / (sqrtf(v) + eps);
}

__global__ __launch_bounds__(256) void adam_tf_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, size_t n,
                                                      float lr_t, float b1, float b2, float eps, float gs) {
    const size_t n4 = n >> 2;
    const float ob1 = 1.0f - b1, ob2 = 1.0f - b2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * gs;
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 wv = reinterpret_cast<f32x4*>(w)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float me = mv[e], ve = vv[e], we = wv[e];       // (element references of an ext-vector miscompile under bit casts: copies)
            adam_elem(we, gv[e], me, ve, lr_t, b1, b2, ob1, ob2, eps);
            mv[e] = me; vv[e] = ve; wv[e] = we;
        }
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        reinterpret_cast<f32x4*>(w)[i] = wv;
    }
    if (blockIdx.x == 0) {
        for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            float mi = m[i], vi = v[i], wi = w[i];
            adam_elem(wi, g[i] * gs, mi, vi, lr_t, b1, b2, ob1, ob2, eps);
            m[i] = mi;
            v[i] = vi;
            w[i] = wi;
        }
    }
}

// The same update with the step count and the learning rate in DEVICE memory, so that a captured HIP graph of a whole train
// step can be replayed without a per-step kernel argument (ESPCN trains for 1.6 M steps of a dozen ~10-us launches,
// espcn/makefile:30-36).  state: { int64 t; float lr; float lr_t (out, for inspection); uint32 blocks_done }.
// Every block reads t BEFORE any block can have changed it: the increment is done by the block that finishes last
// (a counter of finished blocks), i.e. after all of them have read it.  lr_t is evaluated by one thread per block in
// double precision with the same expression as the host path (srx_adam_tf_step).
struct AdamState {
    long long t;
    float lr, lr_t;
    unsigned done, pad;
};
__global__ __launch_bounds__(256) void adam_tf_dev_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, size_t n,
                                                          AdamState* __restrict__ st, float b1, float b2, float eps, float gs) {
    __shared__ float sh_lr_t;
    if (threadIdx.x == 0) {
        const double t = (double)(__atomic_load_n(&st->t, __ATOMIC_RELAXED) + 1);
        sh_lr_t = (float)((double)st->lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    }
    __syncthreads();
    const float lr_t = sh_lr_t;
    const size_t n4 = n >> 2;
    const float ob1 = 1.0f - b1, ob2 = 1.0f - b2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * gs;
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 wv = reinterpret_cast<f32x4*>(w)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float me = mv[e], ve = vv[e], we = wv[e];       // (element references of an ext-vector miscompile under bit casts: copies)
            adam_elem(we, gv[e], me, ve, lr_t, b1, b2, ob1, ob2, eps);
            mv[e] = me; vv[e] = ve; wv[e] = we;
        }
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        reinterpret_cast<f32x4*>(w)[i] = wv;
    }
    if (blockIdx.x == 0) {
        for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            float mi = m[i], vi = v[i], wi = w[i];
            adam_elem(wi, g[i] * gs, mi, vi, lr_t, b1, b2, ob1, ob2, eps);
            m[i] = mi;
            v[i] = vi;
            w[i] = wi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(&st->done, 1u) == gridDim.x - 1) {      // every block has read t: the last one to finish advances it
            st->done = 0;
            st->lr_t = lr_t;
            __atomic_store_n(&st->t, st->t + 1, __ATOMIC_RELAXED);
        }
    }
}

__global__ __launch_bounds__(256) void momentum_clip_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                            float* __restrict__ acc, size_t n, float lr, float mom,
                                                            float cap, float gs) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float gi = g[i] * gs;
        gi = fminf(fmaxf(gi, -cap), cap);
        const float a = mom * acc[i] + gi;
        acc[i] = a;
        w[i] -= lr * a;
    }
}

static int ew_grid(size_t n, int per_thread) {
    size_t nb = (n / per_thread + 255) / 256;
    if (nb < 1) nb = 1;
    return (int)(nb < 2048 ? nb : 2048);
}

hipError_t launch_adam(float* w, const float* g, float* m, float* v, size_t n, float lr_t, float b1, float b2,
                       float eps, float gs, hipStream_t s) {
    hipLaunchKernelGGL(adam_tf_kernel, dim3(ew_grid(n, 4)), dim3(256), 0, s, w, g, m, v, n, lr_t, b1, b2, eps, gs);
    return hipGetLastError();
}

hipError_t launch_adam_dev(float* w, const float* g, float* m, float* v, size_t n, void* state, float b1, float b2,
                           float eps, float gs, hipStream_t s) {
    hipLaunchKernelGGL(adam_tf_dev_kernel, dim3(ew_grid(n, 4)), dim3(256), 0, s, w, g, m, v, n, reinterpret_cast<AdamState*>(state), b1, b2, eps, gs);
    return hipGetLastError();
}

hipError_t launch_momentum(float* w, const float* g, float* acc, size_t n, float lr, float mom, float cap, float gs,
                           hipStream_t s) {
    hipLaunchKernelGGL(momentum_clip_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, w, g, acc, n, lr, mom, cap, gs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// misc elementwise
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      float* __restrict__ dpre, size_t n, int act) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dpre[i] = dy[i] * act_grad_from_y(y[i], act);
}

__global__ __launch_bounds__(256) void affine_kernel(const float* __restrict__ x, float* __restrict__ out, size_t n,
                                                     float a, float b) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    {
#pragma clang fp contract(off)
        const float t = a * x[i];                    // two roundings, like the reference's separate multiply and add
        out[i] = t + b;
    }
}

__global__ __launch_bounds__(256) void saturate_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out,
                                                          size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        // multiply and add rounded separately, as the two TensorFlow ops are (a fused multiply-add rounds once and
        // moves a few values across an integer, i.e. changes the truncated byte)
#pragma clang fp contract(off)
        float v = x[i] * 127.5f;
        v = v + 127.5f;
        v = fminf(fmaxf(v, 0.f), 255.f);
        out[i] = (uint8_t)v;  // truncation toward zero, as tf.saturate_cast
    }
}

__global__ __launch_bounds__(256) void psnr_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                   float* __restrict__ out, size_t per_image, float max_val) {
    __shared__ float sh[4];
    const float* pa = a + (size_t)blockIdx.x * per_image;
    const float* pb = b + (size_t)blockIdx.x * per_image;
    float acc = 0.f;
    for (size_t i = threadIdx.x; i < per_image; i += 256) {
        const float d = pa[i] - pb[i];
        acc += d * d;
    }
    const float t = block_sum(acc, sh);
    if (threadIdx.x == 0)
        out[blockIdx.x] = 20.0f * log10f(max_val) - 10.0f * log10f(t / (float)per_image);
}

// Pixel replication and its gradient.  VEC floats per thread (4 when C is a multiple of 4: 16-byte accesses, a
// wavefront covers whole pixels of the 64-channel tensors); one index decomposition per vector.
template <int VEC>
__global__ __launch_bounds__(256) void upsample_nearest_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               int N, int H, int W, int C, int f) {
    const int CV = C / VEC;
    const size_t total = (size_t)N * H * f * W * f * CV;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int c = (int)(o % CV);
        size_t t = o / CV;
        const int ow = (int)(t % ((size_t)W * f));
        t /= (size_t)W * f;
        const int oh = (int)(t % ((size_t)H * f));
        const int n = (int)(t / ((size_t)H * f));
        const size_t src = (((size_t)n * H + oh / f) * W + ow / f) * CV + c;
        if constexpr (VEC == 4)
            reinterpret_cast<float4*>(out)[o] = reinterpret_cast<const float4*>(in)[src];
        else
            out[o] = in[src];
    }
}

// gradient of the replication: din[n,h,w,c] = sum over the f x f block of dout (rows, then columns, in order)
template <int VEC>
__global__ __launch_bounds__(256) void upsample_nearest_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din,
                                                                   int N, int H, int W, int C, int f) {
    const int CV = C / VEC;
    const size_t total = (size_t)N * H * W * CV;
    const size_t orow = (size_t)W * f * CV;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int c = (int)(o % CV);
        size_t t = o / CV;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        const size_t base = (((size_t)n * H * f + (size_t)h * f) * W * f + (size_t)w * f) * CV + c;
        if constexpr (VEC == 4) {
            float4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) {
                    const float4 v = reinterpret_cast<const float4*>(dout)[base + dy * orow + (size_t)dx * CV];
                    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
                }
            reinterpret_cast<float4*>(din)[o] = acc;
        } else {
            float acc = 0.f;
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) acc += dout[base + dy * orow + (size_t)dx * CV];
            din[o] = acc;
        }
    }
}

// gradient through relu(a_in + b_in) where the two branches' gradients arrive separately:
// out = (y > 0) ? a + b : 0   (residual block: gradient via the skip path + gradient via the conv path)
__global__ __launch_bounds__(256) void add_relu_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ y, float* __restrict__ out, size_t n4,
                                                            size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
        const float4 vy = reinterpret_cast<const float4*>(y)[i];
        float4 r;
        r.x = vy.x > 0.f ? va.x + vb.x : 0.f; r.y = vy.y > 0.f ? va.y + vb.y : 0.f;
        r.z = vy.z > 0.f ? va.z + vb.z : 0.f; r.w = vy.w > 0.f ? va.w + vb.w : 0.f;
        reinterpret_cast<float4*>(out)[i] = r;
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = y[i] > 0.f ? a[i] + b[i] : 0.f;
}

// SRCNN loss: one block per row computes ||pred-target||_2 of that row; a second pass scales.
__global__ __launch_bounds__(256) void rownorm_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      size_t row_len, float* __restrict__ norms) {
    __shared__ float sh[4];
    const float* pa = a + (size_t)blockIdx.x * row_len;
    const float* pb = b + (size_t)blockIdx.x * row_len;
    float acc = 0.f;
    for (size_t i = threadIdx.x; i < row_len; i += 256) {
        const float d = pa[i] - pb[i];
        acc += d * d;
    }
    const float t = block_sum(acc, sh);
    if (threadIdx.x == 0) norms[blockIdx.x] = sqrtf(t);
}

__global__ __launch_bounds__(256) void rownorm_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           size_t rows, size_t row_len, const float* __restrict__ norms,
                                                           float* __restrict__ dpred) {
    const size_t n = rows * row_len;
    const float inv_rows = 1.0f / (float)rows;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float nr = norms[i / row_len];
        dpred[i] = nr > 0.f ? (a[i] - b[i]) * inv_rows / nr : 0.f;
    }
}

// Long rows (SRCNN's crops: 231 x 231 = 53,361 elements per row, 192 rows per batch): one block per row is 192 blocks streaming
// 427 KB each -- latency-bound (92 us for 82 MB).  Rows are cut into chunks of 4,096 elements, one block per chunk writes its
// sum of squares, a second launch adds a row's chunks in order and takes the root.  The partial sums live in the first floats of
// `dpred` (written before the gradient pass overwrites it): no extra workspace in the C ABI.
constexpr int kRowChunk = 4096;
__global__ __launch_bounds__(256) void rownorm_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              size_t row_len, int chunks, float* __restrict__ parts) {
    __shared__ float sh[4];
    const size_t row = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const size_t i0 = (size_t)chunk * kRowChunk, i1 = (i0 + kRowChunk < row_len) ? i0 + kRowChunk : row_len;
    const float* pa = a + row * row_len;
    const float* pb = b + row * row_len;
    float acc = 0.f;
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float d = pa[i] - pb[i];
        acc += d * d;
    }
    const float t = block_sum(acc, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void rownorm_finish_kernel(const float* __restrict__ parts, int chunks, size_t rows,
                                                             float* __restrict__ norms) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float t = 0.f;
    for (int c = 0; c < chunks; ++c) t += parts[row * chunks + c];
    norms[row] = sqrtf(t);
}

hipError_t launch_rownorm_loss(const float* pred, const float* target, size_t rows, size_t row_len, float* loss,
                               float* dpred, float* norms, hipStream_t s) {
    const size_t chunks = (row_len + kRowChunk - 1) / kRowChunk;
    if (dpred && chunks > 1 && rows * chunks < (1u << 30) && rows * chunks <= rows * row_len) {
        hipLaunchKernelGGL(rownorm_partial_kernel, dim3((unsigned)(rows * chunks)), dim3(256), 0, s, pred, target, row_len, (int)chunks, dpred);
        hipLaunchKernelGGL(rownorm_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, dpred, (int)chunks, rows, norms);
    } else {
        hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)rows), dim3(256), 0, s, pred, target, row_len, norms);
    }
    if (loss) hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, s, norms, (int)rows, 1.0f / (float)rows, loss, 0);
    if (dpred)
        hipLaunchKernelGGL(rownorm_grad_kernel, dim3(ew_grid(rows * row_len, 1)), dim3(256), 0, s, pred, target, rows,
                           row_len, norms, dpred);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// SSIM (tf.image.ssim semantics).  One thread per output position and channel evaluates the 11x11
// gaussian-weighted moments directly; evaluation-only code, HBM/L2-bound at image sizes.
// ---------------------------------------------------------------------------------------------
constexpr int kSsimBlocks = 128;   // partial sums per image

__global__ __launch_bounds__(256) void ssim_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           int H, int W, int C, float c1, float c2,
                                                           float* __restrict__ partial) {
    __shared__ float sh[4];
    __shared__ float g[11];
    if (threadIdx.x < 11) {
        float sum = 0.f;
        for (int i = 0; i < 11; ++i) sum += __expf(-(float)((i - 5) * (i - 5)) / (2.0f * 1.5f * 1.5f));
        const int d = (int)threadIdx.x - 5;
        g[threadIdx.x] = __expf(-(float)(d * d) / (2.0f * 1.5f * 1.5f)) / sum;
    }
    __syncthreads();
    const int n = blockIdx.y;
    const int OH = H - 10, OW = W - 10;
    const size_t total = (size_t)OH * OW * C;
    const float* pa = a + (size_t)n * H * W * C;
    const float* pb = b + (size_t)n * H * W * C;
    float acc = 0.f;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int c = (int)(o % C);
        const size_t t = o / C;
        const int ow = (int)(t % OW), oh = (int)(t / OW);
        float ma = 0.f, mb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
        for (int i = 0; i < 11; ++i) {
            const float* ra = pa + ((size_t)(oh + i) * W + ow) * C + c;
            const float* rb = pb + ((size_t)(oh + i) * W + ow) * C + c;
            float xa = 0.f, xb = 0.f, xaa = 0.f, xbb = 0.f, xab = 0.f;
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                const float va = ra[(size_t)j * C], vb = rb[(size_t)j * C], w = g[j];
                xa += w * va; xb += w * vb; xaa += w * va * va; xbb += w * vb * vb; xab += w * va * vb;
            }
            const float wi = g[i];
            ma += wi * xa; mb += wi * xb; saa += wi * xaa; sbb += wi * xbb; sab += wi * xab;
        }
        // TF's _ssim_per_channel: luminance * contrast-structure
        const float num0 = 2.0f * ma * mb, den0 = ma * ma + mb * mb;
        const float lum = (num0 + c1) / (den0 + c1);
        const float cs = (2.0f * sab - num0 + c2) / (saa + sbb - den0 + c2);
        acc += lum * cs;
    }
    const float t = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)n * kSsimBlocks + blockIdx.x] = t;
}

__global__ __launch_bounds__(128) void ssim_finish_kernel(const float* __restrict__ partial, float inv_count,
                                                          float* __restrict__ out) {
    __shared__ double sh[128];
    sh[threadIdx.x] = (threadIdx.x < kSsimBlocks) ? (double)partial[(size_t)blockIdx.x * kSsimBlocks + threadIdx.x] : 0.0;
    __syncthreads();
    for (int o = 64; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(sh[0] * (double)inv_count);
}

size_t ssim_scratch_bytes(int N) { return (size_t)(N > 0 ? N : 0) * kSsimBlocks * sizeof(float); }

hipError_t launch_ssim(const float* a, const float* b, float* out, int N, int H, int W, int C, float max_val,
                       float* scratch, hipStream_t s) {
    const float c1 = (0.01f * max_val) * (0.01f * max_val), c2 = (0.03f * max_val) * (0.03f * max_val);
    hipLaunchKernelGGL(ssim_partial_kernel, dim3(kSsimBlocks, N), dim3(256), 0, s, a, b, H, W, C, c1, c2, scratch);
    const double count = (double)(H - 10) * (W - 10) * C;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(N), dim3(128), 0, s, scratch, (float)(1.0 / count), out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// LR synthesis ("next" row N1): uint8 -> float, separable gaussian blur, bilinear resize
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void u8_to_float_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                          size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = (float)in[i] / 255.0f;
}

// AXIS 0: along H, 1: along W.  Border: replicate (index clamp).
template <int AXIS>
__global__ __launch_bounds__(256) void gaussian_1d_kernel(const float* __restrict__ in, float* __restrict__ out, int N,
                                                          int H, int W, int C, float sigma, int radius) {
    __shared__ float wts[64];
    if (threadIdx.x <= (unsigned)radius && threadIdx.x < 64) {
        float sum = 0.f;
        for (int i = -radius; i <= radius; ++i) sum += expf(-0.5f * (float)(i * i) / (sigma * sigma));
        wts[threadIdx.x] = expf(-0.5f * (float)(threadIdx.x * threadIdx.x) / (sigma * sigma)) / sum;
    }
    __syncthreads();
    const size_t total = (size_t)N * H * W * C;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int c = (int)(o % C);
        size_t t = o / C;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const size_t n = t / H;
        const float* base = in + n * (size_t)H * W * C + c;
        float acc = 0.f;
        for (int i = -radius; i <= radius; ++i) {
            int hh = h, ww = w;
            if (AXIS == 0) { hh = h + i; hh = hh < 0 ? 0 : (hh >= H ? H - 1 : hh); }
            else { ww = w + i; ww = ww < 0 ? 0 : (ww >= W ? W - 1 : ww); }
            acc += wts[i < 0 ? -i : i] * base[((size_t)hh * W + ww) * C];
        }
        out[o] = acc;
    }
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              int N, int H, int W, int C, int OH, int OW) {
    const size_t total = (size_t)N * OH * OW * C;
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int c = (int)(o % C);
        size_t t = o / C;
        const int ow = (int)(t % OW);
        t /= OW;
        const int oh = (int)(t % OH);
        const size_t n = t / OH;
        float fy = ((float)oh + 0.5f) * sy - 0.5f, fx = ((float)ow + 0.5f) * sx - 0.5f;
        fy = fminf(fmaxf(fy, 0.f), (float)(H - 1));
        fx = fminf(fmaxf(fx, 0.f), (float)(W - 1));
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
        const float wy = fy - (float)y0, wx = fx - (float)x0;
        const float* base = in + n * (size_t)H * W * C + c;
        const float v00 = base[((size_t)y0 * W + x0) * C], v01 = base[((size_t)y0 * W + x1) * C];
        const float v10 = base[((size_t)y1 * W + x0) * C], v11 = base[((size_t)y1 * W + x1) * C];
        out[o] = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
    }
}

hipError_t launch_u8_to_float(const uint8_t* in, float* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(u8_to_float_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

hipError_t launch_gaussian_blur(const float* in, float* out, float* tmp, int N, int H, int W, int C, float sigma,
                                hipStream_t s) {
    const size_t total = (size_t)N * H * W * C;
    if (sigma <= 0.f) return hipMemcpyAsync(out, in, total * sizeof(float), hipMemcpyDeviceToDevice, s);
    const int radius = (int)(4.0f * sigma + 0.5f);
    if (radius > 63) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gaussian_1d_kernel<0>, dim3(ew_grid(total, 1)), dim3(256), 0, s, in, tmp, N, H, W, C, sigma, radius);
    hipLaunchKernelGGL(gaussian_1d_kernel<1>, dim3(ew_grid(total, 1)), dim3(256), 0, s, tmp, out, N, H, W, C, sigma, radius);
    return hipGetLastError();
}

hipError_t launch_resize_bilinear(const float* in, float* out, int N, int H, int W, int C, int OH, int OW, hipStream_t s) {
    const size_t total = (size_t)N * OH * OW * C;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(ew_grid(total, 1)), dim3(256), 0, s, in, out, N, H, W, C, OH, OW);
    return hipGetLastError();
}

hipError_t launch_act_bwd(const float* dy, const float* y, float* dpre, size_t n, int act, hipStream_t s) {
    hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, dy, y, dpre, n, act);
    return hipGetLastError();
}
hipError_t launch_affine(const float* x, float* out, size_t n, float a, float b, hipStream_t s) {
    hipLaunchKernelGGL(affine_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, x, out, n, a, b);
    return hipGetLastError();
}
hipError_t launch_saturate_u8(const float* x, uint8_t* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(saturate_u8_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, x, out, n);
    return hipGetLastError();
}
hipError_t launch_psnr(const float* a, const float* b, float* out, int N, size_t per_image, float max_val,
                       hipStream_t s) {
    hipLaunchKernelGGL(psnr_kernel, dim3(N), dim3(256), 0, s, a, b, out, per_image, max_val);
    return hipGetLastError();
}
hipError_t launch_upsample_nearest(const float* in, float* out, int N, int H, int W, int C, int f, hipStream_t s) {
    const bool v4 = (C % 4) == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0;
    const size_t total = (size_t)N * H * f * W * f * (v4 ? C / 4 : C);
    if (v4)
        hipLaunchKernelGGL(upsample_nearest_kernel<4>, dim3(ew_grid(total, 1)), dim3(256), 0, s, in, out, N, H, W, C, f);
    else
        hipLaunchKernelGGL(upsample_nearest_kernel<1>, dim3(ew_grid(total, 1)), dim3(256), 0, s, in, out, N, H, W, C, f);
    return hipGetLastError();
}
hipError_t launch_upsample_nearest_bwd(const float* dout, float* din, int N, int H, int W, int C, int f, hipStream_t s) {
    const bool v4 = (C % 4) == 0 && ((uintptr_t)dout % 16) == 0 && ((uintptr_t)din % 16) == 0;
    const size_t total = (size_t)N * H * W * (v4 ? C / 4 : C);
    if (v4)
        hipLaunchKernelGGL(upsample_nearest_bwd_kernel<4>, dim3(ew_grid(total, 1)), dim3(256), 0, s, dout, din, N, H, W, C, f);
    else
        hipLaunchKernelGGL(upsample_nearest_bwd_kernel<1>, dim3(ew_grid(total, 1)), dim3(256), 0, s, dout, din, N, H, W, C, f);
    return hipGetLastError();
}
hipError_t launch_add_relu_grad(const float* a, const float* b, const float* y, float* out, size_t n, hipStream_t s) {
    const bool v4 = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y | (uintptr_t)out) % 16) == 0;
    const size_t n4 = v4 ? n / 4 : 0;
    hipLaunchKernelGGL(add_relu_grad_kernel, dim3(ew_grid(n4 ? n4 : n, 1)), dim3(256), 0, s, a, b, y, out, n4, n);
    return hipGetLastError();
}

// Test aid (srx_debug_poison_lds): fills the whole LDS of every CU with quiet NaNs.  A kernel that reads LDS it has not written
// -- a pad slot, a zero-weighted operand -- gives the same answer whatever ran before it only if it does not depend on those
// bytes; with the LDS poisoned before every call a dependence shows up as a NaN in the parity tests.
__global__ __launch_bounds__(256) void poison_lds_kernel(int n4) {
    extern __shared__ __attribute__((aligned(16))) float lds_poison[];
    const f32x4 q = {__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000)};
    for (int i = threadIdx.x; i < n4; i += 256) reinterpret_cast<f32x4*>(lds_poison)[i] = q;
    __syncthreads();
    // (read one value back into a side effect nobody sees, so that the stores are not dropped)
    if (lds_poison[(threadIdx.x * 61) % (4 * n4)] == 0.0f) __builtin_amdgcn_s_sleep(1);
}
hipError_t launch_poison_lds(hipStream_t s) {
    // one workgroup fills a CU's whole LDS, so no two share a CU; four rounds' worth of them reach every CU
    return launch_with_lds<poison_lds_kernel>(dim3(1024), dim3(256), kCuLdsBytes, s, kCuLdsBytes / 16);
}

}  // namespace srx
