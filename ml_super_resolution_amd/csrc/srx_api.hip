// srx_api.hip -- the C ABI of libsrx.so (include/srx.h): argument checking, tile planning,
// kernel-instance dispatch.  No device synchronisation, no allocation.  The pair builders' host side is pairs_api.hip.
#include <math.h>
#include <stdarg.h>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/srx.h"
#include "elementwise.h"
#include "launchers.h"
#include "bf16x3.h"
#include "image_scores.h"
#include "dihedral.h"

using namespace srx;

namespace {

thread_local char g_err[512] = "";

// Tuning / A-B knobs from the environment, read ONCE (C++11 function-local statics are initialised thread-safely):
// the ABI promises concurrent calls from several host threads on different streams.
struct Knobs {
    int pipe_default, narrow, wgrad_lin, wgrad_pipe, wgrad_pipe_strip, wgrad_rows_full, wgrad_1x1, wgrad_pack3, kwrows_min_pixels, big_route_min_pixels, strip_d2s, conv_1x1_min_pixels, pack3_dgrad;
    int chain, chain_fixed, wgrad_batch;
    unsigned long long* trace;
    int dbg;
};
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
Knobs read_knobs() {
    Knobs k;
    k.pipe_default = env_int("SRX_PIPE", 1);
    k.narrow = env_int("SRX_NARROW", 1);
    k.wgrad_lin = env_int("SRX_WGRAD_LIN", 1);
    k.wgrad_pipe = env_int("SRX_WGRAD_PIPE", 1);
    k.wgrad_pipe_strip = env_int("SRX_WGRAD_PIPE_STRIP", 1);   // 0: column-strip filter gradients on the two-workgroup kernel (A/B)
    // SRCNN's forward layers on their own kernels (5x5 32->3: conv_kwrows_kernel; 9x9 3->64: conv_pack3_kernel) from this many
    // output pixels (negative: never).  Round 4 started them at 60,000; timed against conv_mfma_kernel they win from the
    // smallest images on (one 100 x 100 image: level; 170 x 170: 42 against 73 us for the three layers)
    k.kwrows_min_pixels = env_int("SRX_KWROWS_MIN_PIXELS", 4096);
    // ESPCN's 5x5 3->64 on conv_pack3_kernel, 3x3 32->27 on conv_rows3x3_kernel (from 150,000), and the 5x5 32->3 filter
    // gradient on wgrad_kwcols_kernel: from this many output pixels (below: the one-launch ESPCN kernel's window and the
    // training patches, measured on the older kernels only)
    k.big_route_min_pixels = env_int("SRX_BIG_ROUTE_MIN_PIXELS", 60000);
    // 1x1 forward / data gradient (32 / 64 channels) on the streaming conv_1x1_kernel from this many pixels (negative: never)
    k.conv_1x1_min_pixels = env_int("SRX_CONV_1X1_MIN_PIXELS", 100000);
    k.pack3_dgrad = env_int("SRX_PACK3_DGRAD", 1);             // 0: the 5x5 32->3 layer's data gradient stays on conv_mfma_kernel (A/B)
    k.strip_d2s = env_int("SRX_STRIP_D2S", 1);                 // 0: ESPCN's f3 on wide images stays off the pipelined strip kernel (A/B)
    k.wgrad_rows_full = env_int("SRX_WGRAD_ROWS_FULL", 1);     // 0: 41-pixel rows on the padded-position walk (wgrad_pipe_kernel) instead of wgrad_rows_full_kernel (A/B)
    k.wgrad_1x1 = env_int("SRX_WGRAD_1X1", 1);                 // 0: 1x1 filter gradients on wgrad_mfma_kernel instead of the streaming wgrad_1x1_kernel (A/B)
    k.wgrad_pack3 = env_int("SRX_WGRAD_PACK3", 1);             // 0: RGB-input 9x9 / 5x5 filter gradients on the cursor kernel's 4-channel rows (A/B)
    k.chain = env_int("SRX_CHAIN", 1);                          // 0: srx_conv_chain refuses every chain; the callers launch per layer (A/B)
    k.chain_fixed = env_int("SRX_CHAIN_FIXED", 1);              // 0: chains of 41-pixel rows run the generic chain instance, not the fixed-geometry one (A/B)
    k.wgrad_batch = env_int("SRX_WGRAD_BATCH", 1);              // 0: srx_conv2d_bwd_filter_batch refuses every batch; the callers launch per layer (A/B)
    k.trace = nullptr;
    k.dbg = 0;
#ifdef SRX_TRACE
    { const char* tp = getenv("SRX_TRACE_PTR"); k.trace = tp ? (unsigned long long*)strtoull(tp, nullptr, 0) : nullptr; }
    k.dbg = env_int("SRX_DBG", 0);                   // diagnostic builds only (make EXTRA=-DSRX_TRACE)
#endif
    return k;
}
const Knobs& knobs() { static const Knobs k = read_knobs(); return k; }

// A runtime switch of the ABI (srx_set_*): -1 = not set by the caller, the environment's default (Dflt) applies.
template <int (*Dflt)()>
struct Toggle {
    std::atomic<int> v{-1};
    int get() const { const int x = v.load(std::memory_order_relaxed); return x < 0 ? Dflt() : x; }
    // sets the caller's value (-1: unsets it) and returns the value in effect before
    int set(int x) { const int old = v.exchange(x, std::memory_order_relaxed); return old < 0 ? Dflt() : old; }
};
inline int on_off(int on) { return on < 0 ? -1 : (on ? 1 : 0); }
inline int pipe_default() { return knobs().pipe_default; }
inline int chain_default() { return knobs().chain ? 1 : 0; }
inline int chain_fixed_default() { return knobs().chain_fixed ? 1 : 0; }
inline int wgrad_batch_default() { return knobs().wgrad_batch ? 1 : 0; }
inline int wgrad_path_default() { return !knobs().wgrad_lin ? 0 : ((knobs().wgrad_pipe || knobs().wgrad_pipe_strip) ? 2 : 1); }
Toggle<pipe_default> g_use_pipe;                  // conv kernel family, see srx_set_conv_path
Toggle<chain_default> g_chain;                    // chained body layers, see srx_set_chain
Toggle<chain_fixed_default> g_chain_fixed;        // fixed-geometry chain instances, see srx_set_chain_fixed
Toggle<wgrad_batch_default> g_wgrad_batch;        // batched body filter gradients, see srx_set_wgrad_batch
Toggle<wgrad_path_default> g_wgrad_path;          // filter-gradient kernel family, see srx_set_wgrad_path
int use_pipe() { return g_use_pipe.get(); }
int wgrad_path() { return g_wgrad_path.get(); }

// Compute units of the current device (persistent-workgroup grids are sized from it): queried once per device.
// Without a device (host-only workspace queries on a build box) the MI355X's 256.
int cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = 256;
    }
    if (n > 256) n = 256;     // grids and partial counts are planned for at most 2 x 256 persistent workgroups
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// a launcher's status as the entry point's return code; `what` is the text in front of the runtime's own
int launch_status(hipError_t err, const char* what) {
    return err == hipSuccess ? SRX_OK : fail(SRX_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(err));
}
}  // namespace
namespace srx {
// the same for the other translation units with extern "C" entry points (pairs_api.hip, enet_ops.hip)
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace srx
namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr size_t kLdsBudget = 80 * 1024 - 336;  // two workgroups per CU (160 KiB); 320 B spare for wgrad's zero slot
constexpr int kMaxGridLimit = 512;        // upper bound of any persistent grid (2 x 256 CUs): sizes the partial-count check
inline int max_grid() { return 2 * cu_count(); }   // two persistent workgroups per CU
inline int pipe_grid() { return cu_count(); }      // pipelined kernels: one persistent workgroup per CU

struct Plan {
    int KH, KW, cinp, nch;
    int pad_t, pad_l, OH, OW;
    int TH, TW, NTX, RS;
    int units_total, grid;
    size_t lds_bytes;
};

// bytes of one pixel slot of an LDS tile: the padded channels plus 4 floats against bank conflicts (Lds<CINP>::PS)
size_t slot_bytes(int cinp) { return (size_t)((cinp == 4) ? 4 : cinp + 4) * 4; }
int pad_channels(int c) { return c <= 4 ? 4 : (c <= 32 ? 32 : (c <= 64 ? 64 : -1)); }
int chunks_for(int c) { return c <= 16 ? 1 : (c <= 32 ? 2 : (c <= 64 ? 4 : -1)); }

// in_c / out_c: channels of the tensor staged through LDS / produced by the kernel.
// (H,W) staged tensor dims, (OH,OW) produced tensor dims, pads relative to the staged tensor.
// lean_epilogue: the launch carries one of the epilogues the one-workgroup-per-CU kernels implement (none / ReLU;
// every dgrad and wgrad) -- only used to tell which kernel family the plan is for.
int make_plan(int N, int H, int W, int OH, int OW, int in_c, int out_c, int KH, int KW, int pad_t, int pad_l,
              Plan* p, bool lean_epilogue = true) {
    p->KH = KH; p->KW = KW;
    p->cinp = pad_channels(in_c);
    p->nch = chunks_for(out_c);
    if (p->cinp < 0 || p->nch < 0)
        return fail(SRX_ERR_UNSUPPORTED, "channel counts %d->%d outside the kernel set (<=64)", in_c, out_c);
    p->pad_t = pad_t; p->pad_l = pad_l; p->OH = OH; p->OW = OW;
    const size_t max_slots = kLdsBudget / slot_bytes(p->cinp);
    // full-width tiles: the zero column(s) left of row r+1 double as the right padding of row r
    int RS = W + pad_l;
    if (RS < OW + KW - 1 - (KW - 1 - pad_l)) RS = OW + pad_l;
    // A tile row holds the OW + KW - 1 input columns from -pad_l on; what does not fit wraps into the next row's
    // pad_l leading zero slots.  Even filter sizes with SAME padding pad one more column AFTER than before (TF:
    // pad_before = (K-1)/2), so their rows need one slot more than W + pad_l (round 2: found by the extended shape
    // sweep -- 2x2 / 4x4 SAME read the next row's first pixel as right padding).
    if (RS < OW + KW - 1 - pad_l) RS = OW + KW - 1 - pad_l;
    int TW = OW, NTX = 1;
    long th_max = ((long)max_slots - (KW - 1)) / RS - (KH - 1);
    const int kMaxGrid = max_grid();
    // full-width tiles of 1-2 rows re-stage 3 input rows per output row: measured slower than column tiles
    if (th_max < 3) {
        // column tiling: each tile carries its own halo columns; narrow the tile until it fits
        for (TW = 32; TW >= 8; TW >>= 1) {
            RS = TW + KW - 1;
            th_max = ((long)max_slots - (KW - 1)) / RS - (KH - 1);
            if (th_max >= 1) break;
        }
        if (th_max < 1) return fail(SRX_ERR_UNSUPPORTED, "filter %dx%d too large for the LDS tile", KH, KW);
        NTX = (OW + TW - 1) / TW;
    }
    if (th_max > OH) th_max = OH;
    if (th_max > 16) th_max = 16;
    // Small problems (fewer than two tallest tiles per workgroup slot): the launch is latency-bound, so pick the tile
    // height that minimises the time of the busiest workgroup instead of the tallest one.  Per tile a workgroup pays
    // one staging round trip (load -> LDS -> barrier, epilogue: ~1.5 units) plus one unit (a 16-pixel sub-tile's MFMA
    // chain over all taps, ~2 us for 3x3x64) per sub-tile its busiest wave owns.  Measured at 32x17x17, 64->32: one-row
    // tiles (the previous rule) 35-39 us per launch.
    const long rows_total = (long)N * NTX * OH;
    bool small = false, rows_split = false;
    if (rows_total / th_max < 2 * kMaxGrid && KH == 3 && KW == 3 && p->cinp >= 16 && in_c == p->cinp && lean_epilogue &&
        (out_c & 3) == 0 && RS >= 256 / (p->cinp / 4) && (NTX > 1 ? p->nch == 4 : 16 * (4 / p->nch) <= OW)) {
        // ... except for the layers the one-workgroup-per-CU kernels take (3x3, exact-fit channels): they stage the next
        // tile under the running one and pay per group, not per tile, so the tallest tile stays best (measured at
        // 64x41x41: 4.57 ms per train step with 5-row tiles, 4.85 with 3, 5.15 with 2); only the row split must
        // still reach every CU.
        rows_split = true;
    } else if (rows_total / th_max < 2 * kMaxGrid) {
        const int npart = 4 / p->nch;
        double best_cost = 1e30;
        int best_th = 1;
        for (int th = 1; th <= (int)th_max; ++th) {
            const long tiles = (long)N * NTX * ((OH + th - 1) / th);
            const long slots = tiles < kMaxGrid ? tiles : kMaxGrid;
            const long per_wg = (tiles + slots - 1) / slots;
            const long sub = ((long)th * TW + 15) / 16;
            const double cost = (double)per_wg * (1.5 + (double)((sub + npart - 1) / npart));
            if (cost <= best_cost + 1e-9) { best_cost = cost; best_th = th; }   // ties: the taller tile (less halo)
        }
        th_max = best_th;
        small = true;
    }
    // among the tallest candidates pick the one wasting the fewest lanes of the 16-pixel sub-tiles
    int best = (int)th_max;
    double best_eff = 0.0;
    for (int th = (int)th_max; !small && th >= (int)((th_max + 1) / 2) && th >= 1; --th) {
        const int px = th * TW;
        const double eff = (double)px / (16.0 * ((px + 15) / 16));
        if (eff > best_eff + 1e-9) { best_eff = eff; best = th; }
    }
    p->TH = best; p->TW = TW; p->NTX = NTX; p->RS = RS;
    p->units_total = (int)rows_total;
    long g = rows_total / p->TH;
    // (small problems: one workgroup per tile -- with tiles-per-image workgroups per image the static row split falls
    // on image boundaries, so no workgroup straddles two images and pays for two tiles)
    if (small) g = (long)N * NTX * ((OH + p->TH - 1) / p->TH);
    if (rows_split) g = rows_total;
    if (g < 1) g = 1;
    p->grid = (int)(g < kMaxGrid ? g : kMaxGrid);
    p->lds_bytes = ((size_t)(p->TH + KH - 1) * RS + (KW - 1)) * slot_bytes(p->cinp);
    return SRX_OK;
}

int check_desc(const srx_conv_desc* d) {
    if (!d) return fail(SRX_ERR_BAD_ARG, "null descriptor");
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->KH <= 0 || d->KW <= 0)
        return fail(SRX_ERR_BAD_ARG, "non-positive dimension in descriptor");
    if (d->stride != 1 && d->stride != 2) return fail(SRX_ERR_UNSUPPORTED, "stride %d: strides 1 and 2 are implemented", d->stride);
    if (d->stride == 2 && d->subpixel_r > 1) return fail(SRX_ERR_UNSUPPORTED, "stride 2 with the sub-pixel store is not implemented");
    if (d->pad_mode != SRX_PAD_SAME && d->pad_mode != SRX_PAD_VALID) return fail(SRX_ERR_BAD_ARG, "bad pad_mode");
    if (d->act < SRX_ACT_NONE || d->act > SRX_ACT_SIGMOID) return fail(SRX_ERR_BAD_ARG, "bad activation");
    if (d->post_add_relu != 0 && d->post_add_relu != SRX_ACT_RELU && d->post_add_relu != SRX_ACT_LRELU)
        return fail(SRX_ERR_BAD_ARG, "post_add_relu must be 0, SRX_ACT_RELU (1) or SRX_ACT_LRELU (3)");
    if (d->precision != SRX_PRECISION_FP32 && d->precision != SRX_PRECISION_BF16X3)
        return fail(SRX_ERR_BAD_ARG, "bad precision %d: 0 (exact fp32) or 1 (bf16x3)", d->precision);
    if (d->subpixel_r < 0 || d->subpixel_r > 16) return fail(SRX_ERR_BAD_ARG, "bad subpixel_r %d", d->subpixel_r);
    if (d->subpixel_r > 1 && d->Cout % (d->subpixel_r * d->subpixel_r))
        return fail(SRX_ERR_BAD_ARG, "subpixel_r %d: Cout %d is not a multiple of r*r", d->subpixel_r, d->Cout);
    if (d->pad_mode == SRX_PAD_VALID && (d->H < d->KH || d->W < d->KW))
        return fail(SRX_ERR_BAD_ARG, "VALID convolution with input smaller than the filter");
    if ((long)d->H * d->W * (long)(d->Cin > d->Cout ? d->Cin : d->Cout) >= (1L << 31))
        return fail(SRX_ERR_UNSUPPORTED, "one image has >= 2^31 elements: beyond the kernels' 32-bit in-image offsets");
    if ((long)d->N * d->H * 64 >= (1L << 31))
        return fail(SRX_ERR_UNSUPPORTED, "too many rows for 32-bit unit indexing");
    return SRX_OK;
}

// TensorFlow's geometry: SAME: out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before = pad_total / 2
// (the odd one goes AFTER: a stride-2 3x3 layer on an even-sized image pads 0 before / 1 after,
// enet/enet/model_enet.py:136-146; on an odd-sized one 1 / 1).  VALID: out = (in - k) / s + 1.
void geometry(const srx_conv_desc* d, int* pad_t, int* pad_l, int* OH, int* OW) {
    const int s = d->stride;
    if (d->pad_mode == SRX_PAD_SAME) {
        *OH = (d->H + s - 1) / s; *OW = (d->W + s - 1) / s;
        const int ph = (*OH - 1) * s + d->KH - d->H, pw = (*OW - 1) * s + d->KW - d->W;
        *pad_t = (ph > 0 ? ph : 0) / 2; *pad_l = (pw > 0 ? pw : 0) / 2;
    } else {
        *pad_t = 0; *pad_l = 0; *OH = (d->H - d->KH) / s + 1; *OW = (d->W - d->KW) / s + 1;
    }
}

// Stride 2 (forward and filter gradient on the two-workgroup kernels): every tile carries its own halo -- RS = (TW - 1) 2 +
// KW slots per tile row, (TH - 1) 2 + KH rows -- and output pixel (r, c) of a tile reads its window at tile slot (2r, 2c).
// Picks the column width that puts the most output pixels into the 80-KiB tile.
int make_plan_s2(int N, int H, int W, int OH, int OW, int in_c, int out_c, int KH, int KW, int pad_t, int pad_l, Plan* p) {
    p->KH = KH; p->KW = KW;
    p->cinp = pad_channels(in_c);
    p->nch = chunks_for(out_c);
    if (p->cinp < 0 || p->nch < 0)
        return fail(SRX_ERR_UNSUPPORTED, "channel counts %d->%d outside the kernel set (<=64)", in_c, out_c);
    p->pad_t = pad_t; p->pad_l = pad_l; p->OH = OH; p->OW = OW;
    const long max_slots = (long)(kLdsBudget / slot_bytes(p->cinp)) - 8;     // (the cursor wgrad kernel keeps a zeroed slot behind the tile)
    int best_tw = 0, best_th = 0;
    long best_px = 0;
    for (int TW = 32; TW >= 4; TW >>= 1) {
        const int tw = TW < OW ? TW : OW;
        const long RS = (long)(tw - 1) * 2 + KW;
        long rows = (max_slots - (KW - 1)) / RS;                 // tile rows that fit
        long th = (rows - KH) / 2 + 1;
        if (rows < KH || th < 1) continue;
        if (th > OH) th = OH;
        if (th > 16) th = 16;
        const long px = th * tw;
        if (px > best_px) { best_px = px; best_tw = tw; best_th = (int)th; }
        if (TW >= OW && TW > 4) continue;
    }
    if (!best_px) return fail(SRX_ERR_UNSUPPORTED, "filter %dx%d at stride 2 too large for the LDS tile", KH, KW);
    p->TW = best_tw; p->TH = best_th;
    p->NTX = (OW + best_tw - 1) / best_tw;
    p->RS = (best_tw - 1) * 2 + KW;
    const long rows_total = (long)N * p->NTX * OH;
    if (rows_total >= (1L << 31)) return fail(SRX_ERR_UNSUPPORTED, "too many rows for 32-bit unit indexing");
    p->units_total = (int)rows_total;
    long g = rows_total / p->TH;
    if (g < 1) g = 1;
    const int kMaxGrid = max_grid();
    p->grid = (int)(g < kMaxGrid ? g : kMaxGrid);
    p->lds_bytes = ((size_t)((p->TH - 1) * 2 + KH) * p->RS + (KW - 1)) * slot_bytes(p->cinp);
    return SRX_OK;
}

// Precision 1 (bf16x3, conv_bf16x3.hip): 3x3 stride-1 SAME 64 -> 64 layers; the forward pass with no activation or
// ReLU and no post-add activation or sub-pixel store.  Depends on the descriptor's layer, never on N, H, W.
// SRX_OK, or SRX_ERR_UNSUPPORTED with the reason.  (The caller has run check_desc.)
int bf16x3_supported(const srx_conv_desc* d, int op) {
    if (d->KH != 3 || d->KW != 3)
        return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): filter %dx%d; only 3x3 layers run at it", d->KH, d->KW);
    if (d->Cin != 64 || d->Cout != 64)
        return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): channels %d->%d; only 64->64 layers run at it", d->Cin, d->Cout);
    if (d->stride != 1) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): stride %d; only stride 1 runs at it", d->stride);
    if (d->pad_mode != SRX_PAD_SAME) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): VALID padding; only SAME runs at it");
    if (d->post_add_relu != 0) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): post_add_relu %d is not implemented", d->post_add_relu);
    if (d->subpixel_r > 1) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): the sub-pixel store (subpixel_r %d) is not implemented", d->subpixel_r);
    if (d->act != SRX_ACT_NONE && d->act != SRX_ACT_RELU)
        return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): activation %d; only none and ReLU run at it", d->act);
    if (op != SRX_OP_FWD && op != SRX_OP_BWD_DATA && op != SRX_OP_BWD_FILTER) return fail(SRX_ERR_BAD_ARG, "bad op %d", op);
    if (!launch_conv3x3c64_bf16x3 || !launch_wgrad3x3c64_bf16x3)
        return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): this build has no bf16x3 kernels");
    return SRX_OK;
}

// Precision 1: tiles of the bf16x3 kernels (conv_bf16x3.hip).  Picks the tile that minimises the modelled time of the
// busiest workgroup: per tile ~20 cycles per staged slot (HBM, conversion, LDS store) plus ~54 per output pixel of MFMA
// work (whole 16- / 32-pixel steps).  Column widths: the image width itself when a tile row of it fits, else 16 .. 64.
void bf16x3_plan(int N, int H, int W, int max_grid, bool wgrad, Bf3Plan* p) {
    const long max_slots = (long)(kBf3Lds / (wgrad ? kBf3WgradSlot : kBf3ConvSlot));
    const int cands[] = {W, 16, 24, 32, 48, 64};
    double best = 1e300;
    *p = Bf3Plan{1, 1, W, H, N * H * W, 1, 0};
    for (int TW : cands) {
        if (TW > W || TW < 1) continue;
        const long RS = TW + 2;
        long fit = wgrad ? (max_slots - 1 - 2 * RS) / (RS + TW) : max_slots / RS - 2;
        if (fit > H) fit = H;
        for (long th = fit; th >= 1; --th) {
            const long ntx = (W + TW - 1) / TW, nty = (H + th - 1) / th, tiles = (long)N * ntx * nty;
            const long px = th * TW, slots = (th + 2) * RS + (wgrad ? 1 + px : 0), step = wgrad ? 32 : 16;
            const double per_tile = 20.0 * slots + 54.0 * ((px + step - 1) / step * step);
            const long grid = tiles < max_grid ? tiles : max_grid;
            const double cost = (double)((tiles + grid - 1) / grid) * per_tile + 1e-3 * (double)tiles * per_tile / grid;
            if (cost < best) {
                best = cost;
                p->TH = (int)th; p->TW = TW; p->ntx = (int)ntx; p->nty = (int)nty; p->tiles = (int)tiles; p->grid = (int)grid;
                p->lds = (size_t)slots * (wgrad ? kBf3WgradSlot : kBf3ConvSlot);
            }
        }
    }
    if (wgrad && p->lds < 256 * 16) p->lds = 256 * 16;   // the bias-gradient reduction
}

size_t part_stride(const srx_conv_desc* d) {
    const size_t per = (size_t)d->KH * d->KW * d->Cin * d->Cout + (size_t)d->Cout;
    return (per + 3) / 4 * 4;
}
size_t partials_bytes(const srx_conv_desc* d, size_t count) { return count * part_stride(d) * sizeof(float); }

// ---- route predicates: each condition under which a kernel family takes a layer, stated once ---------------------------
// (the launchers add their own share: the key they are instantiated for, min_pixels, their size bounds)

// 32-bit byte offsets inside the staged and the produced tensor (the pipelined kernels' buffer addressing)
bool conv_tensors_below_2g(const ConvArgs& a) {
    return (long)a.H * a.W * a.Cin * 4 < (1L << 31) - 64 && (long)a.OH * a.OW * a.Cout * 4 < (1L << 31) - 64;
}

// Epilogue forms the one-workgroup-per-CU kernels implement (integer-VALU only): none / ReLU, ReLU-gradient mask,
// residual add (+ ReLU).
bool pipe_epilogue_ok(const ConvArgs& a, bool wt) {
    return (a.act == ACT_NONE || a.act == ACT_RELU) && (a.post_relu == 0 || a.post_relu == ACT_RELU) && !(a.mask && a.skip) && !(wt && a.skip) && !(!wt && a.mask) &&
           (!a.mask || (a.mask_act == ACT_RELU && a.act == ACT_NONE && !a.post_relu));
}

// The full-width pipelined route (conv_pipe_kernel), epilogue aside.  Its lean staging cursor / sub-tile walk /
// buffer-store epilogue cover: exact-fit channels, full-width tiles, a row stride of at least one staging pass, sub-tile
// steps of at most one row, 16-byte output vectors and images below 2^31 bytes.
// (p.RS == W + pad_l: the only pad slots of a tile row are the pad_l leading ones, which the scalar staging
// never writes; a dgrad of a VALID layer has trailing pad slots inside the row as well and stays on path 0)
// Consumers: dispatch_conv, chain_plan.
bool pipe_full_width_ok(const Plan& p, const ConvArgs& a) {
    const int ppp = 256 / (p.cinp / 4), npart = 4 / p.nch;
    return !a.d2s_r && a.stride == 1 && a.Cin == p.cinp && p.NTX == 1 && p.RS >= ppp && p.RS == a.W + a.pad_l &&
           16 * npart <= a.OW && (a.Cout & 3) == 0 && conv_tensors_below_2g(a);
}

// Column-strip variant of the pipelined kernel (images too wide for full-width tiles): strips of 16 or 32 columns
// no wider than the image, one sub-tile sequence per workgroup (64 output channels); any padding.
// Consumer: dispatch_conv.
bool pipe_strip_ok(const Plan& p, const ConvArgs& a, bool wt) {
    const int ppp = 256 / (p.cinp / 4), npart = 4 / p.nch;
    // (32 output channels: forward only, no aux operand, and the one shape with a tanh form of the deferred epilogue -- ESPCN's f2)
    const bool strip2 = npart == 2 && !wt && !a.skip && !a.mask && !a.post_relu && a.Cout == 32 && p.cinp == 64 &&
                        (a.act == ACT_NONE || a.act == ACT_RELU || a.act == ACT_TANH);
    // (ESPCN's f3 -- 3x3 32 -> 3 r^2 through the sub-pixel map, no activation -- on the same two-chunk strips: AUX = 4.
    // Its epilogue addresses an RGB image, 3 r floats per pixel of an output row: Cout must BE 3 r^2 -- among 17..32
    // that is 27 with r = 3.  32 -> 32 with r = 2 or 4 was taken too and stored to the addresses of a 3-channel image.)
    const bool strip_d2s = knobs().strip_d2s && npart == 2 && !wt && !a.skip && !a.mask && !a.post_relu && a.d2s_r > 0 && a.act == ACT_NONE &&
                           p.cinp == 32 && a.Cout > 16 && a.Cout <= 32 && a.Cout == 3 * a.d2s_r * a.d2s_r && p.KH == 3 && p.KW == 3 &&
                           (long)a.OH * a.d2s_r * a.OW * a.d2s_r * 3 * 4 < (1L << 31) - 64;
    return (pipe_epilogue_ok(a, wt) || strip2 || strip_d2s) && (!a.d2s_r || strip_d2s) && a.stride == 1 && a.Cin == p.cinp && p.NTX > 1 &&
           (p.TW == 16 || p.TW == 32) && a.OW >= p.TW &&
           p.RS >= ppp && (npart == 1 || strip2 || strip_d2s) && ((a.Cout & 3) == 0 || strip_d2s) &&
           a.y != a.skip && a.y != a.mask &&   // (the columns two strips share are computed twice: no in-place epilogue operand)
           conv_tensors_below_2g(a);
}

// ---- forward / data gradient: the ladder of offers ----------------------------------------------------------------------
// Each launcher answers whether the key (and its own bounds) is its; the first that takes the layer ends the ladder.
// srx_set_conv_path(0) / SRX_PIPE=0 keeps every shape on the conv_mfma_kernel family at the bottom: the reference
// point of the bit-identity tests (conv_pack3 / conv_1x1 / conv_rows3x3 are bit-identical to it, conv_kwrows agrees to
// rounding: the kw partial sums are added in another order).
int dispatch_conv(const Plan& p, bool wt, const ConvArgs& a_in, hipStream_t s) {
    ConvKey k{p.KH, p.KW, p.cinp, p.nch, wt};
    hipError_t err = hipSuccess;
    ConvArgs a = a_in;
    const Knobs& kn = knobs();
    const bool pipe = use_pipe() != 0;
    const long pack3_min = k.kh == 9 ? kn.kwrows_min_pixels : kn.big_route_min_pixels;
    const auto taken = [&err] { return launch_status(err, "conv launch failed"); };   // (the launcher that takes the layer ends the ladder)
    // three output channels (the RGB output layer): 16 lanes per pixel, no MFMA -- conv_narrow.hip; SRX_NARROW=0 for A/B
    if (kn.narrow && !a.d2s_r && a.stride == 1 && launch_conv_narrow(k, a, s, &err)) return taken();
    // SRCNN's 5x5 32 -> 3: (kw, co) pairs as the MFMA's rows -- conv_kwrows.hip; RGB-input 9x9 / 5x5: (kw, ci) along K -- conv_pack3.hip
    if (pipe && kn.kwrows_min_pixels >= 0 && launch_conv_kwrows(k, a, kn.kwrows_min_pixels, s, &err)) return taken();
    if (pipe && kn.kwrows_min_pixels >= 0 && (!k.wt || kn.pack3_dgrad) && launch_conv_pack3(k, a, pack3_min, s, &err)) return taken();
    // 1x1 layers on large inputs: HBM-bound, no LDS -- conv_1x1.hip
    if (pipe && kn.conv_1x1_min_pixels >= 0 && launch_conv_1x1(k, a, kn.conv_1x1_min_pixels, s, &err)) return taken();
    // The 3x3 body layers: the pipelined one-wave-per-SIMD kernels (measured 7 % faster than the two-workgroups-per-CU
    // kernels at 256x41x41x64), full-width tiles or column strips; every later offer sees their buffer size too.
    const bool body = pipe && p.cinp >= 16, strips = body && pipe_strip_ok(p, a, wt), full = body && pipe_epilogue_ok(a, wt) && pipe_full_width_ok(p, a);
    const int pgrid = p.grid < pipe_grid() ? p.grid : pipe_grid();   // pipelined kernels: one workgroup per CU, two LDS tile buffers
    if (strips || full) a.buf_floats = (int)(p.lds_bytes / 4);
    if (strips && launch_pipe_strip(k, a, pgrid, 2 * p.lds_bytes, s, &err)) return taken();
    if (full && launch_pipe_k3c64(k, a, pgrid, 2 * p.lds_bytes, s, &err)) return taken();
    if (full && launch_pipe_other(k, a, pgrid, 2 * p.lds_bytes, s, &err)) return taken();
    // 3x3 layers of 17..32 output channels that the pipelined family did not take, on large inputs (ESPCN's f2 / f3 on
    // whole images): one workgroup of 8 waves per CU -- conv_rows3x3.hip
    if (pipe && kn.big_route_min_pixels >= 0 && launch_conv_rows3x3(k, a, kn.big_route_min_pixels, s, &err)) return taken();
    // two workgroups per CU: conv_mfma_kernel
    if (launch_conv_k3c64(k, a, p.grid, p.lds_bytes, s, &err)) return taken();
    if (launch_conv_k3c32(k, a, p.grid, p.lds_bytes, s, &err)) return taken();
    if (launch_conv_c4(k, a, p.grid, p.lds_bytes, s, &err)) return taken();
    if (launch_conv_misc(k, a, p.grid, p.lds_bytes, s, &err)) return taken();
    if (launch_conv_generic(k, a, p.grid, p.lds_bytes, s, &err)) return taken();
    return fail(SRX_ERR_UNSUPPORTED, "no kernel instance for %dx%d, Cin<=%d, Cout chunks %d, %s", p.KH, p.KW,
                p.cinp, p.nch, wt ? "dgrad" : "fwd");
}

// Precision 1, forward and data gradient: plan, launch, status
int bf16x3_conv(const srx_conv_desc* d, bool dgrad, const float* x, const float* w, const float* bias, const float* mask, bool relu,
                float* y, hipStream_t s) {
    Bf3Plan bp;
    bf16x3_plan(d->N, d->H, d->W, max_grid(), false, &bp);
    return launch_status(launch_conv3x3c64_bf16x3(dgrad, x, w, bias, mask, relu, y, d->N, d->H, d->W, bp, s), "conv launch failed");
}

// s_sleep(127) iterations (~3.4 us each) by which the second workgroup of a CU is delayed; only
// worth it when every CU really hosts two long-running workgroups.
int stagger_sleeps(const Plan& p) {
    if (p.grid < max_grid()) return 0;
    const long tiles_per_wg = (long)p.units_total / ((long)p.grid * p.TH);
    return tiles_per_wg >= 2 ? 4 : 0;
}

// The linear-walk filter-gradient kernels keep 4 zeroed slots behind the tile (their last step may read past it): a
// plan whose tile fills the 80-KiB budget to the last slot (32-wide rows, 64 channels: 7 + 2 rows of 33 slots) would send
// the layer to the cursor kernel (the EnhanceNet generator's residual blocks at 64 x 32 x 32; at that size either kernel
// takes 58 us -- the launch is latency-bound -- but larger batches of such rows are not).  One row less and it fits.  The grid (= number of partial filters = workspace size) does not depend on the tile height.
void wgrad_tile_for_linear_walk(const srx_conv_desc* d, Plan* p) {
    if (p->NTX != 1 || wgrad_path() < 1) return;
    while (p->TH > 1 && p->lds_bytes + 4 * slot_bytes(p->cinp) > 80 * 1024) {
        p->TH -= 1;
        p->lds_bytes = ((size_t)(p->TH + d->KH - 1) * p->RS + (d->KW - 1)) * slot_bytes(p->cinp);
    }
}

// ---- planning: the one way from a descriptor and an op to a tile plan ---------------------------------------------------
struct LayerPlan {
    Plan p;
    int pt, pl, OH, OW;            // the layer's geometry, in the forward sense
    int N, H, W, in_c, out_c;      // the tensor the kernel stages through LDS; the channels it stages / produces
};

// Forward and filter gradient stage x [N,H,W,Cin]; the data gradient stages dpre [N,OH,OW,Cout] and produces dx
// [N,H,W,Cin] with full-correlation padding.  What differs between the entry points is a parameter:
//   lean_epilogue     make_plan's hint: the forward pass sets it from the activation, every other caller passes true;
//   linear_walk_tile  shorten a stride-1 filter-gradient tile for the linear-walk kernels' zeroed slots; every
//                     filter-gradient entry point but srx_conv2d_workspace_bytes does (the grid, and so the workspace,
//                     does not depend on the tile height).
int plan_layer(const srx_conv_desc* d, int op, bool lean_epilogue, bool linear_walk_tile, LayerPlan* lp) {
    geometry(d, &lp->pt, &lp->pl, &lp->OH, &lp->OW);
    const bool dgrad = op == SRX_OP_BWD_DATA;
    lp->N = d->N;
    lp->H = dgrad ? lp->OH : d->H; lp->W = dgrad ? lp->OW : d->W;
    lp->in_c = dgrad ? d->Cout : d->Cin; lp->out_c = dgrad ? d->Cin : d->Cout;
    int rc;
    if (dgrad) rc = make_plan(d->N, lp->OH, lp->OW, d->H, d->W, d->Cout, d->Cin, d->KH, d->KW, d->KH - 1 - lp->pt, d->KW - 1 - lp->pl, &lp->p, lean_epilogue);
    else if (d->stride == 2) rc = make_plan_s2(d->N, d->H, d->W, lp->OH, lp->OW, d->Cin, d->Cout, d->KH, d->KW, lp->pt, lp->pl, &lp->p);
    else rc = make_plan(d->N, d->H, d->W, lp->OH, lp->OW, d->Cin, d->Cout, d->KH, d->KW, lp->pt, lp->pl, &lp->p, lean_epilogue);
    if (rc == SRX_OK && linear_walk_tile && d->stride != 2) wgrad_tile_for_linear_walk(d, &lp->p);
    return rc;
}

void fill_conv_args(ConvArgs* a, const LayerPlan& lp) {
    const Plan& p = lp.p;
    a->N = lp.N; a->H = lp.H; a->W = lp.W; a->OH = p.OH; a->OW = p.OW; a->Cin = lp.in_c; a->Cout = lp.out_c;
    a->pad_t = p.pad_t; a->pad_l = p.pad_l;
    a->TH = p.TH; a->TW = p.TW; a->NTX = p.NTX; a->RS = p.RS;
    a->units_total = p.units_total;
    a->inv_rs = 1.0f / (float)p.RS;
    a->stride = 1;
    a->stagger = stagger_sleeps(p);
    a->dbg = knobs().dbg;        // both zero / null unless built with -DSRX_TRACE
    a->trace = knobs().trace;
}

// Chained body layers (conv_chain.hip): the plan and arguments of one layer of a chain, or SRX_ERR_UNSUPPORTED with the
// reason.  Eligible: the exact 3x3 64 -> 64 stride-1 SAME layer on the full-width conv_pipe_kernel route with the
// epilogue it implements (forward: none / ReLU, no skip; data gradient: no mask, or a ReLU-gradient mask), and N a
// multiple of the pipelined grid, so that every workgroup's row range is whole images.
int chain_plan(const srx_conv_desc* d, int op, int in_act, LayerPlan* lp, ConvArgs* a, int* grid) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (op != SRX_OP_FWD && op != SRX_OP_BWD_DATA) return fail(SRX_ERR_BAD_ARG, "chain: op %d (forward or data gradient)", op);
    if (!g_chain.get()) return fail(SRX_ERR_UNSUPPORTED, "chain: switched off (srx_set_chain / SRX_CHAIN)");
    if (!use_pipe()) return fail(SRX_ERR_UNSUPPORTED, "chain: conv path 0");
    if (!launch_conv_chain) return fail(SRX_ERR_UNSUPPORTED, "chain: this build has no chain kernels");
    if (d->precision != SRX_PRECISION_FP32) return fail(SRX_ERR_UNSUPPORTED, "chain: precision %d (exact fp32 only)", d->precision);
    if (d->KH != 3 || d->KW != 3 || d->Cin != 64 || d->Cout != 64 || d->stride != 1 || d->pad_mode != SRX_PAD_SAME)
        return fail(SRX_ERR_UNSUPPORTED, "chain: only 3x3 64->64 stride-1 SAME layers");
    if (d->subpixel_r > 1 || d->post_add_relu) return fail(SRX_ERR_UNSUPPORTED, "chain: no sub-pixel store or post-add activation");
    if (op == SRX_OP_FWD && d->act != SRX_ACT_NONE && d->act != SRX_ACT_RELU)
        return fail(SRX_ERR_UNSUPPORTED, "chain: forward activation %d (none / ReLU)", d->act);
    if (op == SRX_OP_BWD_DATA && in_act != SRX_ACT_NONE && in_act != SRX_ACT_RELU)
        return fail(SRX_ERR_UNSUPPORTED, "chain: in_act %d (none / ReLU)", in_act);
    if ((rc = plan_layer(d, op, true, false, lp)) != SRX_OK) return rc;
    const Plan& p = lp->p;
    memset(a, 0, sizeof(*a));
    fill_conv_args(a, *lp);
    a->act = (op == SRX_OP_FWD) ? d->act : SRX_ACT_NONE;
    a->post_relu = 0;
    a->mask_act = (op == SRX_OP_FWD) ? 0 : in_act;
    a->trace = nullptr;
    // dispatch_conv's route to conv_pipe_kernel<3, 3, 64, 4, ...> (the epilogue forms were checked above, with their own texts)
    if (!(p.cinp == 64 && p.nch == 4 && pipe_full_width_ok(p, *a)))
        return fail(SRX_ERR_UNSUPPORTED, "chain: the shape is not on the full-width pipelined route (column strips?)");
    *grid = p.grid < pipe_grid() ? p.grid : pipe_grid();
    if (d->N % *grid) return fail(SRX_ERR_UNSUPPORTED, "chain: N %d is not a multiple of the grid %d (a workgroup would split an image)", d->N, *grid);
    a->buf_floats = (int)(p.lds_bytes / 4);
    return SRX_OK;
}

}  // namespace

extern "C" {

int srx_set_chain(int on) { return g_chain.set(on_off(on)); }
int srx_set_chain_fixed(int on) { return g_chain_fixed.set(on_off(on)); }

int srx_conv_chain_supported(const srx_conv_desc* d, int op, int in_act) {
    LayerPlan lp;
    ConvArgs a;
    int grid;
    return chain_plan(d, op, in_act, &lp, &a, &grid) == SRX_OK ? 1 : 0;
}

int srx_conv_chain(const srx_conv_desc* d, int op, int in_act, int layers, const float* const* x, const float* const* w,
                   const float* const* bias, const float* const* aux, float* const* y, srx_stream_t stream) {
    if (layers < 1 || layers > kChainMax) return fail(SRX_ERR_BAD_ARG, "chain: %d layers (1..%d)", layers, kChainMax);
    if (!x || !w || !y) return fail(SRX_ERR_BAD_ARG, "null pointer array");
    LayerPlan lp;
    ConvArgs a;
    int grid;
    int rc = chain_plan(d, op, in_act, &lp, &a, &grid);
    if (rc) return rc;
    const bool wt = op == SRX_OP_BWD_DATA;
    const bool masked = wt && in_act == SRX_ACT_RELU;
    ChainPtrs c;
    memset(&c, 0, sizeof(c));
    c.L = layers;
    for (int l = 0; l < layers; ++l) {
        const float* m = aux ? aux[l] : nullptr;
        if (!x[l] || !w[l] || !y[l]) return fail(SRX_ERR_BAD_ARG, "chain: null tensor pointer in layer %d", l);
        if (!wt && m) return fail(SRX_ERR_UNSUPPORTED, "chain: the forward skip operand is not implemented");
        if (masked != (m != nullptr)) return fail(SRX_ERR_BAD_ARG, "chain: layer %d: a mask goes with in_act ReLU, and only with it", l);
        if (!aligned16(x[l]) || !aligned16(w[l]) || !aligned16(y[l]) || (m && !aligned16(m)) || (bias && bias[l] && (reinterpret_cast<uintptr_t>(bias[l]) & 3)))
            return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
        if (y[l] == x[l] || (m && y[l] == m)) return fail(SRX_ERR_BAD_ARG, "chain: layer %d writes its own operand", l);
        c.x[l] = x[l]; c.w[l] = w[l]; c.bias[l] = (bias && !wt) ? bias[l] : nullptr; c.aux[l] = m; c.y[l] = y[l];
    }
    return launch_status(launch_conv_chain(wt, masked, g_chain_fixed.get() != 0, a, c, grid, 2 * lp.p.lds_bytes, (hipStream_t)stream),
                         "chain launch failed");
}

const char* srx_version(void) { return "srx 0.1 (gfx950, fp32 MFMA 16x16x4)"; }
const char* srx_last_error(void) { return g_err; }
int srx_set_conv_path(int pipelined) { return g_use_pipe.set(pipelined ? 1 : 0); }   // (no "unset": any value but 0 is the pipelined family)
int srx_set_wgrad_path(int path) { return g_wgrad_path.set(path < 0 ? -1 : (path > 2 ? 2 : path)); }
size_t srx_reduce_scratch_bytes(void) { return (size_t)kReduceBlocks * sizeof(float); }

int srx_conv2d_precision_supported(const srx_conv_desc* d, int op) {
    if (check_desc(d) != SRX_OK) return 0;
    if (op != SRX_OP_FWD && op != SRX_OP_BWD_DATA && op != SRX_OP_BWD_FILTER) { fail(SRX_ERR_BAD_ARG, "bad op %d", op); return 0; }
    if (d->precision == SRX_PRECISION_FP32) return 1;
    return bf16x3_supported(d, op) == SRX_OK ? 1 : 0;
}

size_t srx_conv2d_workspace_bytes(const srx_conv_desc* d, int op) {
    if (check_desc(d) != SRX_OK) return 0;
    if (d->precision == SRX_PRECISION_BF16X3) {
        if (bf16x3_supported(d, op) != SRX_OK) return 0;
        if (op != SRX_OP_BWD_FILTER) return 256;   // (unused by the bf16x3 kernels; the same optional size as precision 0)
        Bf3Plan bp;
        bf16x3_plan(d->N, d->H, d->W, max_grid(), true, &bp);
        return partials_bytes(d, bp.grid);
    }
    if (op != SRX_OP_BWD_FILTER) return 256;   // reserved: FWD / BWD_DATA do not use their workspace
    LayerPlan lp;
    if (plan_layer(d, SRX_OP_BWD_FILTER, true, false, &lp) != SRX_OK) return 0;
    return partials_bytes(d, lp.p.grid);
}

int srx_conv2d_fwd(const srx_conv_desc* d, const float* x, const float* w, const float* bias, const float* skip,
                   float* y, void* /*ws: reserved*/, size_t /*ws_bytes*/, srx_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !w || !y) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (!aligned16(x) || !aligned16(w) || !aligned16(y) || (skip && !aligned16(skip)))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    if (d->precision == SRX_PRECISION_BF16X3) {
        if ((rc = bf16x3_supported(d, SRX_OP_FWD)) != SRX_OK) return rc;
        if (skip) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): the skip operand is not implemented");
        return bf16x3_conv(d, false, x, w, bias, nullptr, d->act == SRX_ACT_RELU, y, (hipStream_t)stream);
    }
    LayerPlan lp;
    if ((rc = plan_layer(d, SRX_OP_FWD, d->act == SRX_ACT_NONE || d->act == SRX_ACT_RELU, false, &lp)) != SRX_OK) return rc;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = w; a.bias = bias; a.skip = skip; a.mask = nullptr; a.y = y;
    fill_conv_args(&a, lp);
    a.act = d->act; a.post_relu = d->post_add_relu; a.mask_act = 0;
    a.stride = d->stride;
    if (d->subpixel_r > 1) {
        // the store goes through the depth-to-space map: y is [N, OH*r, OW*r, Cout/(r*r)]
        if (skip) return fail(SRX_ERR_UNSUPPORTED, "subpixel_r with a skip operand is not implemented");
        a.d2s_r = d->subpixel_r;
        a.d2s_rc = d->Cout / d->subpixel_r;
    }
    return dispatch_conv(lp.p, false, a, (hipStream_t)stream);
}

static int bwd_data_impl(const srx_conv_desc* d, const float* dpre, const float* w, const float* x_in, int in_act,
                         const float* dx_acc, float* dx_out, srx_stream_t stream);

int srx_conv2d_bwd_data(const srx_conv_desc* d, const float* dpre, const float* w, const float* x_in, int in_act,
                        float* dx_out, void* /*ws: reserved*/, size_t /*ws_bytes*/, srx_stream_t stream) {
    return bwd_data_impl(d, dpre, w, x_in, in_act, nullptr, dx_out, stream);
}

int srx_conv2d_bwd_data_acc(const srx_conv_desc* d, const float* dpre, const float* w, const float* dx_acc, float* dx_out,
                            void* /*ws: reserved*/, size_t /*ws_bytes*/, srx_stream_t stream) {
    if (!dx_acc) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    return bwd_data_impl(d, dpre, w, nullptr, SRX_ACT_NONE, dx_acc, dx_out, stream);
}

static int bwd_data_impl(const srx_conv_desc* d, const float* dpre, const float* w, const float* x_in, int in_act,
                         const float* dx_acc, float* dx_out, srx_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!dpre || !w || !dx_out) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (!aligned16(dpre) || !aligned16(w) || !aligned16(dx_out) || (x_in && !aligned16(x_in)) || (dx_acc && !aligned16(dx_acc)))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    if (in_act < SRX_ACT_NONE || in_act > SRX_ACT_SIGMOID) return fail(SRX_ERR_BAD_ARG, "bad in_act");
    if (d->stride != 1)
        return fail(SRX_ERR_UNSUPPORTED, "bwd_data at stride %d: the data gradient of a stride-2 layer is the stride-1 data gradient of the "
                                         "zero-stuffed upstream gradient (srx_subsample2_bwd, then this entry point with stride 1)", d->stride);
    if (d->precision == SRX_PRECISION_BF16X3) {
        if ((rc = bf16x3_supported(d, SRX_OP_BWD_DATA)) != SRX_OK) return rc;
        if (dx_acc) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): srx_conv2d_bwd_data_acc is not implemented");
        if (x_in && in_act != SRX_ACT_NONE && in_act != SRX_ACT_RELU)
            return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): in_act %d; only none and ReLU run at it", in_act);
        return bf16x3_conv(d, true, dpre, w, nullptr, in_act == SRX_ACT_RELU ? x_in : nullptr, false, dx_out, (hipStream_t)stream);
    }
    LayerPlan lp;
    if ((rc = plan_layer(d, SRX_OP_BWD_DATA, true, false, &lp)) != SRX_OK) return rc;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dpre; a.w = w; a.bias = nullptr; a.skip = dx_acc; a.mask = x_in; a.y = dx_out;
    fill_conv_args(&a, lp);
    a.act = SRX_ACT_NONE; a.post_relu = 0; a.mask_act = in_act;
    return dispatch_conv(lp.p, true, a, (hipStream_t)stream);
}

namespace {
// Everything of a filter-gradient launch but its pointers; no stagger and no trace (the per-layer entry sets both).
void fill_wgrad_args(WgradArgs* a, const srx_conv_desc* d, const LayerPlan& lp) {
    const Plan& p = lp.p;
    memset(a, 0, sizeof(*a));
    a->part_stride = (int)part_stride(d);
    a->N = d->N; a->H = d->H; a->W = d->W; a->OH = lp.OH; a->OW = lp.OW; a->Cin = d->Cin; a->Cout = d->Cout;
    a->pad_t = lp.pt; a->pad_l = lp.pl; a->TH = p.TH; a->TW = p.TW; a->NTX = p.NTX; a->RS = p.RS;
    a->units_total = p.units_total; a->inv_rs = 1.0f / (float)p.RS;
    a->stride = d->stride;
    a->zero_slot = ((p.TH - 1) * d->stride + d->KH) * p.RS + (d->KW - 1);      // first slot after the largest tile
}

// The linear-walk filter-gradient kernels (wgrad_lin_kernel and the kernels built on its walk).  wpath: the filter-
// gradient path (0 cursor kernel, 1 two-workgroup linear walk, 2 one-workgroup pipelined), read once by the caller.
// Stride 2 stays on the cursor kernel, whose pixel cursor simply steps two slots.
size_t wgrad_lin_lds(const Plan& p) { return p.lds_bytes + 4 * slot_bytes(p.cinp); }   // (its last step may read up to 3 slots past the tile: they are allocated and zeroed, their dpre operand is 0)
int wgrad_wppp(const Plan& p) { return (p.cinp >= 16) ? 256 / (p.cinp / 4) : 256; }     // positions of one staging pass

// Full-width tiles.  The LDS bound is NOT part of it: the two-workgroup kernels need wgrad_lin_lds(p) <= 80 KiB, the
// one-workgroup kernels twice that within 160 KiB or a size of their own -- each consumer states its bound.
// Consumers: srx_conv2d_bwd_filter_partials, wgrad_rows_full_ok, pairs_route.
bool wgrad_lin_ok(const srx_conv_desc* d, const LayerPlan& lp, int wpath) {
    const Plan& p = lp.p;
    return wpath >= 1 && d->stride != 2 && p.NTX == 1 && lp.OW >= 4 && p.RS >= 8 && p.RS == d->W + lp.pl &&
           (long)p.TH * lp.OW * d->Cout * 4 < (1L << 30) && (long)d->H * d->W * d->Cin * 4 < (1L << 31) - 4096;
}

// Column strips: exact-fit channels and a tile row of at least one staging pass (the strip stager is the scalar one)
// (and every strip, the narrower last one included, at least one 4-position step wide: the lanes of a step that
// fall into the next tile row are taken to be real positions).
// Consumers: srx_conv2d_bwd_filter_partials, pairs_route (which spelled out OW >= 4 and RS >= 8 as well: both follow
// from NTX > 1 with TW >= 4 and from RS >= wppp >= 16).
bool wgrad_lin_strip_ok(const srx_conv_desc* d, const LayerPlan& lp, int wpath) {
    const Plan& p = lp.p;
    const int wppp = wgrad_wppp(p);
    return wpath >= 1 && d->stride != 2 && p.NTX > 1 && d->Cin == p.cinp && p.RS >= wppp && p.TW >= 4 && wgrad_lin_lds(p) <= 80 * 1024 &&
           (lp.OW % p.TW == 0 || lp.OW % p.TW >= 4) && p.RS <= 3 * wppp &&
           (long)d->H * d->W * d->Cin * 4 < (1L << 31) - 4096 && (long)lp.OH * lp.OW * d->Cout * 4 < (1L << 30);
}

// Column strips on one workgroup per CU with two tile buffers, exact rows (wgrad_rows_strip_kernel): a 32-column strip
// row is 8 whole steps, so the K loop walks real pixels only -- no fake positions, any last-strip width >= 1;
// SRX_WGRAD_PIPE_STRIP=0 / srx_set_wgrad_path(1) keep the two-workgroup padded walk (A/B).
// Consumer: srx_conv2d_bwd_filter_partials.
bool wgrad_rows_strip_ok(const srx_conv_desc* d, const LayerPlan& lp, int wpath) {
    const Plan& p = lp.p;
    return wpath >= 2 && knobs().wgrad_pipe_strip && d->stride != 2 && p.NTX > 1 && p.TW == 32 && p.RS == 32 + d->KW - 1 &&
           d->Cin == p.cinp && 2 * wgrad_lin_lds(p) <= 160 * 1024 &&
           (long)d->H * d->W * d->Cin * 4 < (1L << 31) - 4096 && (long)lp.OH * lp.OW * d->Cout * 4 < (1L << 30);
}

// 41-pixel rows (the VDSR patch of BASELINE's metric): exact rows, one 31-step window per 3-row unit
// (wgrad_rows_full_kernel).  SRX_WGRAD_PIPE=0 / SRX_WGRAD_ROWS_FULL=0 / srx_set_wgrad_path(< 2) keep the layer off it (A/B).
// Consumers: srx_conv2d_bwd_filter_partials, wgrad_batch_plan (which reports the switches on their own first).
bool wgrad_rows_full_switches(int wpath) { return wpath >= 2 && knobs().wgrad_pipe && knobs().wgrad_rows_full; }
bool wgrad_rows_full_ok(const srx_conv_desc* d, const LayerPlan& lp, int wpath) {
    return wgrad_rows_full_switches(wpath) && wgrad_lin_ok(d, lp, wpath) && d->KH == 3 && d->KW == 3 && d->Cin == 64 && d->Cout == 64 &&
           lp.OW == 41 && d->W == 41 && lp.pl == 1 && lp.pt == 1 && lp.p.RS == 42;
}
// ... and its launch geometry: returns the LDS bytes of the launch (two tile buffers)
size_t set_wgrad_rows_full_tile(WgradArgs* a) {
    a->TH = 3;                                  // units of 3 rows: one window of 31 steps
    a->zero_slot = (3 + 3) * 42 + 2;            // (a tile row more than the unit needs: the column step's idle lane group reads it)
    return 2 * (size_t)(a->zero_slot + 4) * (64 + 4) * 4;
}

// wgrad_pipe_kernel's step loop runs whole windows of 14 steps (4 positions each), padding a unit's last window with
// zero-operand steps: the tile height that wastes the fewest (41-wide rows: 4 rows = 168 positions = 3 windows
// exactly) while the padded walk stays inside the tile buffer; 0 if every height wastes more than a tenth.
int wgrad_pipe_tile_height(const Plan& p, int zero_slot) {
    const int kWin = 14 * 4;
    int best_th = 0;
    double best_waste = 1e9;
    for (int th = p.TH; th >= 1; --th) {
        const long pos = (long)th * p.RS, padded = (pos + kWin - 1) / kWin * kWin;
        const double waste = (double)(padded - pos) / (double)pos;
        const bool fits = padded + 2L * p.RS + 6 <= (long)zero_slot + 4;
        if (fits && waste < best_waste - 1e-9) { best_waste = waste; best_th = th; }
    }
    return best_waste <= 0.10 ? best_th : 0;
}
}  // namespace

// The filter gradient's ladder of offers: like dispatch_conv's, but an offer may change the number of partial filters.
int srx_conv2d_bwd_filter_partials(const srx_conv_desc* d, const float* x, const float* dpre, void* ws, size_t ws_bytes,
                                   int* n_partials, srx_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !dpre || !n_partials) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (!aligned16(x) || !aligned16(dpre)) return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (d->precision == SRX_PRECISION_BF16X3) {
        if ((rc = bf16x3_supported(d, SRX_OP_BWD_FILTER)) != SRX_OK) return rc;
        Bf3Plan bp;
        bf16x3_plan(d->N, d->H, d->W, max_grid(), true, &bp);
        const size_t need = partials_bytes(d, bp.grid);
        if (!ws || ws_bytes < need) return fail(SRX_ERR_WORKSPACE, "bwd_filter needs %zu workspace bytes, got %zu", need, ws_bytes);
        if (!aligned16(ws)) return fail(SRX_ERR_ALIGN, "workspace must be 16-byte aligned");
        rc = launch_status(launch_wgrad3x3c64_bf16x3(x, dpre, (float*)ws, (int)part_stride(d), d->N, d->H, d->W, bp, s), "wgrad launch failed");
        if (rc == SRX_OK) *n_partials = bp.grid;
        return rc;
    }
    LayerPlan lp;
    if ((rc = plan_layer(d, SRX_OP_BWD_FILTER, true, true, &lp)) != SRX_OK) return rc;
    const Plan& p = lp.p;
    const bool s2 = d->stride == 2;
    const size_t need = partials_bytes(d, p.grid);
    if (!ws || ws_bytes < need)
        return fail(SRX_ERR_WORKSPACE, "bwd_filter needs %zu workspace bytes, got %zu", need, ws_bytes);
    if (!aligned16(ws)) return fail(SRX_ERR_ALIGN, "workspace must be 16-byte aligned");
    WgradArgs a;
    fill_wgrad_args(&a, d, lp);
    a.x = x; a.dpre = dpre;
    a.part = (float*)ws;
    a.stagger = stagger_sleeps(p);
    a.trace = knobs().trace;   // diagnostic builds only
    ConvKey k{d->KH, d->KW, p.cinp, p.nch, false};
    hipError_t err = hipSuccess;
    const Knobs& kn = knobs();
    const int wpath = wgrad_path();                     // 0 cursor kernel, 1 two-workgroup linear walk, 2 one-workgroup pipelined (default)
    const bool lin_ok = wgrad_lin_ok(d, lp, wpath);
    const size_t wg_lds = p.lds_bytes + slot_bytes(p.cinp), lin_lds = wgrad_lin_lds(p);
    const int pgrid = p.grid < pipe_grid() ? p.grid : pipe_grid();   // one workgroup per CU, two tile buffers
    int n1 = 0;
    // (the launcher that takes the layer ends the ladder; `grid`: the partial filters it writes)
    const auto taken = [&err, n_partials](int grid) {
        const int rc = launch_status(err, "wgrad launch failed");
        if (rc == SRX_OK) *n_partials = grid;
        return rc;
    };
    // 1x1 layers (SRCNN 64 -> 32, EnhanceNet's residual blocks 64 -> 64): a streaming GEMM over the pixels, no LDS tile
    if (kn.wgrad_1x1 && wpath >= 1 && !s2 && launch_wgrad_1x1(k, a, p.grid, &n1, s, &err)) return taken(n1);
    // SRCNN's 5x5 32 -> 3 layer on large inputs: (kw, co) pairs as the MFMA's columns (conv_kwrows.hip)
    if (kn.big_route_min_pixels >= 0 && wpath >= 1 && !s2 && launch_wgrad_kwcols(k, a, p.grid, kn.big_route_min_pixels, &n1, s, &err)) return taken(n1);
    if (wgrad_rows_full_ok(d, lp, wpath)) {
        WgradArgs ap = a;
        const size_t lds = set_wgrad_rows_full_tile(&ap);
        if (launch_wgrad_rows_full(k, ap, pgrid, lds, s, &err)) return taken(pgrid);
    }
    // wgrad_pipe_kernel: exact-fit channels, a row stride of at least one pass; SRX_WGRAD_PIPE=0 keeps the two-workgroup kernel (A/B)
    if (wpath >= 2 && kn.wgrad_pipe && lin_ok && d->Cin == p.cinp && p.RS >= wgrad_wppp(p) && 2 * lin_lds <= 160 * 1024) {
        WgradArgs ap = a;
        ap.TH = wgrad_pipe_tile_height(p, a.zero_slot);
        if (ap.TH > 0 && launch_wgrad_pipe(k, ap, pgrid, 2 * lin_lds, s, &err)) return taken(pgrid);
    }
    // 64 <-> 3 channel layers: 16 lanes per position, no MFMA (conv_narrow.hip); SRX_NARROW=0 for A/B
    if (kn.narrow && !s2 && launch_wgrad_narrow(k, a, p.grid, s, &err)) return taken(p.grid);
    if (wgrad_rows_strip_ok(d, lp, wpath) && launch_wgrad_rows_strip(k, a, pgrid, 2 * lin_lds, s, &err)) return taken(pgrid);
    // two workgroups per CU: the linear walk (RGB input: 4-channel rows packed), then the cursor kernel
    if (kn.wgrad_pack3 && lin_ok && lin_lds <= 80 * 1024 && d->Cin == 3 && launch_wgrad_lin_pack3(k, a, p.grid, lin_lds, s, &err)) return taken(p.grid);
    if (wgrad_lin_strip_ok(d, lp, wpath) && launch_wgrad_lin_strip(k, a, p.grid, lin_lds, s, &err)) return taken(p.grid);
    if (lin_ok && lin_lds <= 80 * 1024 && launch_wgrad_lin(k, a, p.grid, lin_lds, s, &err)) return taken(p.grid);
    if (launch_wgrad(k, a, p.grid, wg_lds, s, &err)) return taken(p.grid);
    if (wg_lds <= 80 * 1024 && launch_wgrad_generic(k, a, p.grid, wg_lds, s, &err)) return taken(p.grid);
    return fail(SRX_ERR_UNSUPPORTED, "no wgrad instance for %dx%d, Cin<=%d, Cout chunks %d%s", d->KH, d->KW, p.cinp,
                p.nch, s2 ? " at stride 2" : "");
}

int srx_conv2d_bwd_filter_reduce(const srx_conv_desc* d, const void* ws, int n_partials, float* dw, float* dbias,
                                 const float* w_for_decay, float wd_scale, srx_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!ws || !dw) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (d->precision == SRX_PRECISION_BF16X3 && (rc = bf16x3_supported(d, SRX_OP_BWD_FILTER)) != SRX_OK) return rc;
    if (n_partials <= 0 || n_partials > kMaxGridLimit) return fail(SRX_ERR_BAD_ARG, "bad partial count %d", n_partials);
    const size_t wn = (size_t)d->KH * d->KW * d->Cin * d->Cout;
    return launch_status(launch_reduce_partials((const float*)ws, n_partials, (int)part_stride(d), (int)wn, d->Cout, dw, dbias,
                                                w_for_decay, wd_scale, (hipStream_t)stream), "reduce launch failed");
}

int srx_conv2d_bwd_filter(const srx_conv_desc* d, const float* x, const float* dpre, float* dw, float* dbias,
                          const float* w_for_decay, float wd_scale, void* ws, size_t ws_bytes, srx_stream_t stream) {
    if (!dw) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    int n = 0;
    const int rc = srx_conv2d_bwd_filter_partials(d, x, dpre, ws, ws_bytes, &n, stream);
    if (rc) return rc;
    return srx_conv2d_bwd_filter_reduce(d, ws, n, dw, dbias, w_for_decay, wd_scale, stream);
}

// ---- the filter gradients of several layers of one shape in one launch (wgrad_batch.hip) ------------------------------
namespace {
// Eligible: exactly the layers srx_conv2d_bwd_filter_partials sends to wgrad_rows_full_kernel (precision 0, 3x3 64 -> 64,
// stride 1, SAME, 41-pixel rows, filter-gradient path 2), 2 .. kChainMax of them.  *wpl workgroups per layer: as many as the
// pipelined grid holds for all layers at once, at most one per row.  SRX_OK, or SRX_ERR_UNSUPPORTED with the reason.
// *lds: the LDS bytes of the launch.
int wgrad_batch_plan(const srx_conv_desc* d, int layers, WgradArgs* a, int* wpl, int* grid, size_t* lds) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!g_wgrad_batch.get()) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: switched off (srx_set_wgrad_batch / SRX_WGRAD_BATCH)");
    if (!launch_wgrad_rows_batch || !launch_wgrad_batch_reduce) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: this build has no batch kernels");
    if (layers < 2 || layers > kChainMax) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: %d layers (2..%d)", layers, kChainMax);
    if (d->precision != SRX_PRECISION_FP32) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: precision %d (exact fp32 only)", d->precision);
    if (d->KH != 3 || d->KW != 3 || d->Cin != 64 || d->Cout != 64 || d->stride != 1 || d->pad_mode != SRX_PAD_SAME)
        return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: only 3x3 64->64 stride-1 SAME layers");
    if (d->W != 41) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: W %d (only 41-pixel rows: wgrad_rows_full_kernel's shape)", d->W);
    const int wpath = wgrad_path();
    if (!wgrad_rows_full_switches(wpath))
        return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: the filter-gradient path is not wgrad_rows_full_kernel's (srx_set_wgrad_path)");
    LayerPlan lp;
    if ((rc = plan_layer(d, SRX_OP_BWD_FILTER, true, true, &lp)) != SRX_OK) return rc;
    if (!wgrad_rows_full_ok(d, lp, wpath)) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: the shape is not on wgrad_rows_full_kernel's route");
    const long rows = (long)d->N * lp.OH;
    long w = pipe_grid() / layers;
    if (w > rows) w = rows;
    if (w < 1) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: %d layers on a grid of %d", layers, pipe_grid());
    *wpl = (int)w;
    *grid = pipe_grid();
    fill_wgrad_args(a, d, lp);
    *lds = set_wgrad_rows_full_tile(a);        // as the per-layer launch
    return SRX_OK;
}
}  // namespace

int srx_set_wgrad_batch(int on) { return g_wgrad_batch.set(on_off(on)); }

int srx_conv2d_bwd_filter_batch_plan(const srx_conv_desc* d, int n_layers, int* wgs_per_layer, int* grid) {
    WgradArgs a;
    int wpl = 0, g = 0;
    size_t lds;
    const int rc = wgrad_batch_plan(d, n_layers, &a, &wpl, &g, &lds);
    if (rc) { wpl = 0; g = 0; }
    if (wgs_per_layer) *wgs_per_layer = wpl;
    if (grid) *grid = g;
    return rc;
}

size_t srx_conv2d_bwd_filter_batch_workspace_bytes(const srx_conv_desc* d, int n_layers) {
    WgradArgs a;
    int wpl = 0, g = 0;
    size_t lds;
    if (wgrad_batch_plan(d, n_layers, &a, &wpl, &g, &lds) != SRX_OK) return 0;
    return partials_bytes(d, (size_t)n_layers * wpl);
}

int srx_conv2d_bwd_filter_batch(const srx_conv_desc* d, int n_layers, const float* const* x, const float* const* dpre, float* const* dw,
                                float* const* dbias, const float* const* w_for_decay, float wd_scale, void* ws, size_t ws_bytes,
                                srx_stream_t stream) {
    WgradArgs a;
    int wpl = 0, g = 0;
    size_t lds;
    int rc = wgrad_batch_plan(d, n_layers, &a, &wpl, &g, &lds);
    if (rc) return rc;
    if (!x || !dpre || !dw) return fail(SRX_ERR_BAD_ARG, "null pointer array");
    WgradBatchPtrs c;
    WgradBatchOut o;
    memset(&c, 0, sizeof(c));
    memset(&o, 0, sizeof(o));
    for (int l = 0; l < n_layers; ++l) {
        if (!x[l] || !dpre[l] || !dw[l]) return fail(SRX_ERR_BAD_ARG, "bwd_filter_batch: null tensor pointer in layer %d", l);
        float* const db = dbias ? dbias[l] : nullptr;
        const float* const wl = w_for_decay ? w_for_decay[l] : nullptr;
        if (!aligned16(x[l]) || !aligned16(dpre[l]) || !aligned16(dw[l]) || (db && !aligned16(db)) || (wl && !aligned16(wl)))
            return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: layer %d: every pointer must be 16-byte aligned", l);
        c.x[l] = x[l]; c.dpre[l] = dpre[l];
        o.dw[l] = dw[l]; o.dbias[l] = db; o.w[l] = wl;
    }
    const size_t need = partials_bytes(d, (size_t)n_layers * wpl);
    if (!ws || ws_bytes < need) return fail(SRX_ERR_WORKSPACE, "bwd_filter_batch needs %zu workspace bytes, got %zu", need, ws_bytes);
    if (!aligned16(ws)) return fail(SRX_ERR_UNSUPPORTED, "bwd_filter_batch: the workspace must be 16-byte aligned");
    a.part = (float*)ws;
    if ((rc = launch_status(launch_wgrad_rows_batch(a, c, wpl, n_layers, lds, (hipStream_t)stream), "wgrad batch launch failed")) != SRX_OK) return rc;
    return launch_status(launch_wgrad_batch_reduce((const float*)ws, wpl, n_layers, a.part_stride, d->KH * d->KW * d->Cin * d->Cout, d->Cout, o,
                                                   wd_scale, (hipStream_t)stream), "reduce launch failed");
}

// ---- layers wider than 64 channels: the filter gradients of all (input block, output block) pairs -------------------
namespace {
void blocked_desc(srx_conv_desc* d, int N, int H, int W) {
    memset(d, 0, sizeof(*d));
    d->N = N; d->H = H; d->W = W; d->Cin = 64; d->Cout = 64; d->KH = 3; d->KW = 3; d->stride = 1; d->pad_mode = SRX_PAD_SAME;
}
// One launch for all pairs needs the linear-walk kernel (two workgroups per CU; full-width tiles, or column strips under
// the conditions of the single-layer entry point); G partials per pair so that pairs x G fills the chip about once.
// Returns 0 (one launch per pair), 1 (full-width tiles) or 2 (column strips).
int pairs_route(const srx_conv_desc* d, const LayerPlan& lp, int pairs, int* G) {
    const int wpath = wgrad_path();
    int g = max_grid() / pairs;
    if (g < 1) g = 1;
    if (g > lp.p.grid) g = lp.p.grid;
    *G = g;
    if (pairs <= 1 || pairs > 65535) return 0;
    return (wgrad_lin_ok(d, lp, wpath) && wgrad_lin_lds(lp.p) <= 80 * 1024) ? 1 : (wgrad_lin_strip_ok(d, lp, wpath) ? 2 : 0);
}
// the one pair at a time of the blocked entry points: odd shapes, a single pair, more pairs than one launch's grid
int blocked_pairs_one_by_one(const srx_conv_desc* d, const float* x, const float* dpre, float* dw, float* dbias, int staged_blocks,
                             int produced_blocks, void* ws, size_t ws_bytes, srx_stream_t stream) {
    const size_t blk = (size_t)d->N * d->H * d->W * 64, wn = (size_t)9 * 64 * 64;
    for (int ib = 0; ib < staged_blocks; ++ib)
        for (int ob = 0; ob < produced_blocks; ++ob) {
            const int rc = srx_conv2d_bwd_filter(d, x + ib * blk, dpre + ob * blk, dw + ((size_t)ib * produced_blocks + ob) * wn,
                                                 (ib == 0 && dbias) ? dbias + ob * 64 : nullptr, nullptr, 0.f, ws, ws_bytes, stream);
            if (rc) return rc;
        }
    return SRX_OK;
}
}  // namespace

// Precision 1: the tiles of all pairs' workgroups (G per pair, so that pairs x G fills the chip about once), and the
// workspace of the pairs launch or, beyond one launch's pair count, of the per-pair fallback at precision 1.
static void bf16x3_pairs_plan(int N, int H, int W, int pairs, Bf3Plan* p) {
    int g = max_grid() / pairs;
    if (g < 1) g = 1;
    bf16x3_plan(N, H, W, g, true, p);
}
static size_t bf16x3_pairs_workspace(int N, int H, int W, int pairs) {
    srx_conv_desc d;
    blocked_desc(&d, N, H, W);
    Bf3Plan one, all;
    bf16x3_plan(N, H, W, max_grid(), true, &one);
    bf16x3_pairs_plan(N, H, W, pairs, &all);
    const size_t a = partials_bytes(&d, (size_t)pairs * all.grid), b = partials_bytes(&d, one.grid);
    return pairs > 65535 ? b : (a > b ? a : b);
}

size_t srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(int N, int H, int W, int staged_blocks, int produced_blocks, int precision) {
    if (precision == SRX_PRECISION_FP32) return srx_conv3x3_blocked_bwd_filter_workspace_bytes(N, H, W, staged_blocks, produced_blocks);
    if (precision != SRX_PRECISION_BF16X3) return 0;
    srx_conv_desc d;
    blocked_desc(&d, N, H, W);
    if (check_desc(&d) || staged_blocks <= 0 || produced_blocks <= 0) return 0;
    return bf16x3_pairs_workspace(N, H, W, staged_blocks * produced_blocks);
}

int srx_conv3x3_blocked_bwd_filter_ex(const float* x, const float* dpre, float* dw, float* dbias, int N, int H, int W,
                                      int staged_blocks, int produced_blocks, int precision, void* ws, size_t ws_bytes,
                                      srx_stream_t stream) {
    if (precision != SRX_PRECISION_FP32 && precision != SRX_PRECISION_BF16X3)
        return fail(SRX_ERR_BAD_ARG, "bad precision %d: 0 (exact fp32) or 1 (bf16x3)", precision);
    if (precision == SRX_PRECISION_FP32)
        return srx_conv3x3_blocked_bwd_filter(x, dpre, dw, dbias, N, H, W, staged_blocks, produced_blocks, ws, ws_bytes, stream);
    if (!x || !dpre || !dw) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (staged_blocks <= 0 || produced_blocks <= 0) return fail(SRX_ERR_BAD_ARG, "non-positive block count");
    srx_conv_desc d;
    blocked_desc(&d, N, H, W);
    d.precision = SRX_PRECISION_BF16X3;
    int rc = check_desc(&d);
    if (rc) return rc;
    if ((rc = bf16x3_supported(&d, SRX_OP_BWD_FILTER)) != SRX_OK) return rc;
    if (!launch_wgrad3x3c64_bf16x3_pairs) return fail(SRX_ERR_UNSUPPORTED, "precision 1 (bf16x3): this build has no bf16x3 kernels");
    if (!aligned16(x) || !aligned16(dpre) || !aligned16(dw) || !aligned16(ws) || !aligned16(dbias))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    const int pairs = staged_blocks * produced_blocks;
    const size_t need = bf16x3_pairs_workspace(N, H, W, pairs);
    if (!ws || ws_bytes < need) return fail(SRX_ERR_WORKSPACE, "blocked bwd_filter needs %zu workspace bytes, got %zu", need, ws_bytes);
    // beyond one launch's grid: one pair at a time on the single-layer entry point at precision 1
    if (pairs > 65535) return blocked_pairs_one_by_one(&d, x, dpre, dw, dbias, staged_blocks, produced_blocks, ws, ws_bytes, stream);
    Bf3Plan bp;
    bf16x3_pairs_plan(N, H, W, pairs, &bp);
    const int stride = (int)part_stride(&d);
    if ((rc = launch_status(launch_wgrad3x3c64_bf16x3_pairs(x, dpre, (float*)ws, stride, staged_blocks, produced_blocks, N, H, W, bp, (hipStream_t)stream),
                            "blocked wgrad launch failed")) != SRX_OK) return rc;
    return launch_status(launch_reduce_partials_pairs((const float*)ws, bp.grid, stride, 9 * 64 * 64, 64, dw, dbias, pairs, produced_blocks,
                                                      (hipStream_t)stream), "blocked reduce launch failed");
}

size_t srx_conv3x3_blocked_bwd_filter_workspace_bytes(int N, int H, int W, int staged_blocks, int produced_blocks) {
    srx_conv_desc d;
    blocked_desc(&d, N, H, W);
    if (check_desc(&d) || staged_blocks <= 0 || produced_blocks <= 0) return 0;
    LayerPlan lp;
    if (plan_layer(&d, SRX_OP_BWD_FILTER, true, true, &lp)) return 0;
    int G;
    const int pairs = staged_blocks * produced_blocks;
    const size_t one = partials_bytes(&d, lp.p.grid);
    if (!pairs_route(&d, lp, pairs, &G)) return one;
    const size_t all = partials_bytes(&d, (size_t)pairs * G);
    return all > one ? all : one;
}

int srx_conv3x3_blocked_bwd_filter(const float* x, const float* dpre, float* dw, float* dbias, int N, int H, int W,
                                   int staged_blocks, int produced_blocks, void* ws, size_t ws_bytes, srx_stream_t stream) {
    if (!x || !dpre || !dw) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (staged_blocks <= 0 || produced_blocks <= 0) return fail(SRX_ERR_BAD_ARG, "non-positive block count");
    srx_conv_desc d;
    blocked_desc(&d, N, H, W);
    int rc = check_desc(&d);
    if (rc) return rc;
    if (!aligned16(x) || !aligned16(dpre) || !aligned16(dw) || !aligned16(ws))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    const size_t need = srx_conv3x3_blocked_bwd_filter_workspace_bytes(N, H, W, staged_blocks, produced_blocks);
    if (!ws || ws_bytes < need) return fail(SRX_ERR_WORKSPACE, "blocked bwd_filter needs %zu workspace bytes, got %zu", need, ws_bytes);
    // (32-wide rows: the plan's 7 + 2 rows of 33 slots fill the 80-KiB budget to the last slot and the linear-walk kernel's
    // zeroed slots no longer fit -- every pair would become its own launch; one row less, as on the single-layer entry)
    LayerPlan lp;
    if ((rc = plan_layer(&d, SRX_OP_BWD_FILTER, true, true, &lp)) != SRX_OK) return rc;
    const int pairs = staged_blocks * produced_blocks;
    int G;
    const int route = pairs_route(&d, lp, pairs, &G);
    // one pair at a time on the single-layer entry point (odd shapes, a single pair)
    if (!route) return blocked_pairs_one_by_one(&d, x, dpre, dw, dbias, staged_blocks, produced_blocks, ws, ws_bytes, stream);
    WgradPairs q;
    memset(&q, 0, sizeof(q));
    fill_wgrad_args(&q.a, &d, lp);
    q.a.x = x; q.a.dpre = dpre;
    q.a.part = (float*)ws;
    q.x_pair_stride = q.d_pair_stride = (long)((size_t)N * H * W * 64);
    q.part_pair_stride = (long)G * q.a.part_stride;
    q.cob = produced_blocks;
    ConvKey k{3, 3, 64, 4, false};
    hipError_t err = hipSuccess;
    if (!launch_wgrad_lin_pairs(k, q, G, pairs, route == 2, wgrad_lin_lds(lp.p), (hipStream_t)stream, &err))
        return fail(SRX_ERR_UNSUPPORTED, "no pairs instance of the linear-walk wgrad kernel");
    if ((rc = launch_status(err, "blocked wgrad launch failed")) != SRX_OK) return rc;
    return launch_status(launch_reduce_partials_pairs((const float*)ws, G, q.a.part_stride, 9 * 64 * 64, 64, dw, dbias, pairs, produced_blocks,
                                                      (hipStream_t)stream), "blocked reduce launch failed");
}

#define SRX_CHECK_LAUNCH(expr, what)                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(SRX_ERR_LAUNCH, what ": %s", hipGetErrorString(e_)); \
        return SRX_OK;                                                                       \
    } while (0)

int srx_act_bwd(const float* dy, const float* y, float* dpre, size_t numel, int act, srx_stream_t stream) {
    if (!dy || !y || !dpre) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (act < SRX_ACT_NONE || act > SRX_ACT_SIGMOID) return fail(SRX_ERR_BAD_ARG, "bad activation");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_act_bwd(dy, y, dpre, numel, act, (hipStream_t)stream), "act_bwd");
}

static int subpixel(const float* in, float* out, int N, int H, int W, int C, int r, bool inv, srx_stream_t stream) {
    if (!in || !out) return fail(SRX_ERR_BAD_ARG, "null tensor pointer");
    if (N < 0 || H < 0 || W < 0 || C <= 0 || r <= 0) return fail(SRX_ERR_BAD_ARG, "bad sub-pixel dims");
    if (!aligned16(in) || !aligned16(out)) return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    if (in == out) return fail(SRX_ERR_BAD_ARG, "sub-pixel map cannot run in place");
    if (N == 0 || H == 0 || W == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_subpixel(in, out, N, H, W, C, r, inv, 4 * cu_count(), (hipStream_t)stream), "sub-pixel map");
}

int srx_stream_copy(const void* in, void* out, size_t bytes, srx_stream_t stream) {
    if (!in || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (!aligned16(in) || !aligned16(out) || (bytes & 15u)) return fail(SRX_ERR_ALIGN, "stream copy moves whole 16-byte vectors");
    if (bytes == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_stream_copy((const float*)in, (float*)out, bytes, (hipStream_t)stream), "stream copy");
}

int srx_depth_to_space(const float* in, float* out, int N, int H, int W, int C, int r, srx_stream_t stream) {
    return subpixel(in, out, N, H, W, C, r, false, stream);
}
int srx_space_to_depth(const float* in, float* out, int N, int H, int W, int C, int r, srx_stream_t stream) {
    return subpixel(in, out, N, H, W, C, r, true, stream);
}

int srx_mse_fwd_bwd(const float* pred, const float* target, size_t numel, float inv_numel, float* loss_out,
                    int accumulate, float* dpred, void* scratch, srx_stream_t stream) {
    if (!pred || !target || !scratch) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (!aligned16(pred) || !aligned16(target) || (dpred && !aligned16(dpred)))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_mse(pred, target, numel, inv_numel, loss_out, accumulate, dpred, (float*)scratch,
                                (hipStream_t)stream), "mse");
}

int srx_l2_loss(const float* w, const float* mask, size_t numel, float scale, float* loss_out, int accumulate,
                void* scratch, srx_stream_t stream) {
    if (!w || !loss_out || !scratch) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (!aligned16(w) || (mask && !aligned16(mask)))
        return fail(SRX_ERR_ALIGN, "tensor base pointers must be 16-byte aligned");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_l2(w, mask, numel, scale, loss_out, accumulate, (float*)scratch, (hipStream_t)stream), "l2");
}

int srx_adam_tf_step(float* w, const float* g, float* m, float* v, size_t numel, float lr, float beta1, float beta2,
                     float eps, int64_t t, float grad_scale, srx_stream_t stream) {
    if (!w || !g || !m || !v) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (t < 1) return fail(SRX_ERR_BAD_ARG, "Adam step count t must be >= 1");
    if (!aligned16(w) || !aligned16(g) || !aligned16(m) || !aligned16(v))
        return fail(SRX_ERR_ALIGN, "flat buffers must be 16-byte aligned");
    if (numel == 0) return SRX_OK;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t));
    SRX_CHECK_LAUNCH(launch_adam(w, g, m, v, numel, (float)lr_t, beta1, beta2, eps, grad_scale, (hipStream_t)stream),
                     "adam");
}

int srx_adam_tf_step_dev(float* w, const float* g, float* m, float* v, size_t numel, void* state, float beta1, float beta2,
                         float eps, float grad_scale, srx_stream_t stream) {
    if (!w || !g || !m || !v || !state) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (!aligned16(w) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(state))
        return fail(SRX_ERR_ALIGN, "flat buffers and the state block must be 16-byte aligned");
    if (numel == 0) return fail(SRX_ERR_BAD_ARG, "adam (device state): empty parameter buffer (the step count would not advance)");
    SRX_CHECK_LAUNCH(launch_adam_dev(w, g, m, v, numel, state, beta1, beta2, eps, grad_scale, (hipStream_t)stream), "adam (device state)");
}

int srx_momentum_clip_step(float* w, const float* g, float* acc, size_t numel, float lr, float momentum, float cap,
                           float grad_scale, srx_stream_t stream) {
    if (!w || !g || !acc) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_momentum(w, g, acc, numel, lr, momentum, cap, grad_scale, (hipStream_t)stream), "momentum");
}

int srx_rownorm_loss_fwd_bwd(const float* pred, const float* target, size_t rows, size_t row_len, float* loss_out,
                             float* dpred, float* row_norms, srx_stream_t stream) {
    if (!pred || !target || !row_norms) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (rows == 0 || row_len == 0 || rows > (1u << 30)) return fail(SRX_ERR_BAD_ARG, "bad row-norm dims");
    SRX_CHECK_LAUNCH(launch_rownorm_loss(pred, target, rows, row_len, loss_out, dpred, row_norms, (hipStream_t)stream),
                     "rownorm loss");
}

int srx_psnr(const float* a, const float* b, float* out, int N, size_t per_image, float max_val, srx_stream_t stream) {
    if (!a || !b || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || per_image == 0) return fail(SRX_ERR_BAD_ARG, "bad psnr dims");
    SRX_CHECK_LAUNCH(launch_psnr(a, b, out, N, per_image, max_val, (hipStream_t)stream), "psnr");
}

size_t srx_ssim_scratch_bytes(int N) { return ssim_scratch_bytes(N); }

int srx_ssim(const float* a, const float* b, float* out, int N, int H, int W, int C, float max_val, void* scratch,
             srx_stream_t stream) {
    if (!a || !b || !out || !scratch) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || C <= 0 || H < 11 || W < 11) return fail(SRX_ERR_BAD_ARG, "ssim needs N, C > 0 and H, W >= 11 (11x11 windows)");
    if (N > 65535) return fail(SRX_ERR_UNSUPPORTED, "ssim: more than 65535 images per call");
    SRX_CHECK_LAUNCH(launch_ssim(a, b, out, N, H, W, C, max_val, (float*)scratch, (hipStream_t)stream), "ssim");
}

// The descriptor checks of the three srx_image_scores* functions and the plan they share: the effective row (RL floats, tap
// stride Ce) and the tile counts.  `who` prefixes the message.
struct ScoresPlan {
    int RL, Ce, tiles_y, tiles_x;
};
static int image_scores_plan(const char* who, const srx_scores_desc* d, ScoresPlan* p) {
    if (!d) return fail(SRX_ERR_BAD_ARG, "%s: null descriptor", who);
    if (d->N < 1 || d->N > kScoresMaxN) return fail(SRX_ERR_BAD_ARG, "%s: N %d outside 1..%d (one grid row per image)", who, d->N, kScoresMaxN);
    if (d->C < 1) return fail(SRX_ERR_BAD_ARG, "%s: C %d is below 1", who, d->C);
    if (d->n_cand < 1 || d->n_cand > SRX_SCORES_MAX_CAND) return fail(SRX_ERR_BAD_ARG, "%s: n_cand %d outside 1..%d", who, d->n_cand, SRX_SCORES_MAX_CAND);
    if (d->space != SRX_SCORES_RGB && d->space != SRX_SCORES_Y) return fail(SRX_ERR_BAD_ARG, "%s: space %d is not 0 (rgb) or 1 (y)", who, d->space);
    if (d->space == SRX_SCORES_Y && d->C % 3 != 0) return fail(SRX_ERR_BAD_ARG, "%s: the y space needs C %% 3 == 0, got C %d", who, d->C);
    if (d->unit_clip != 0 && d->unit_clip != 1) return fail(SRX_ERR_BAD_ARG, "%s: unit_clip %d is not 0 or 1", who, d->unit_clip);
    if (!isfinite(d->max_val) || !(d->max_val > 0.0f)) return fail(SRX_ERR_BAD_ARG, "%s: max_val %g is not a finite number above 0", who, (double)d->max_val);
    const long long row_in = (long long)d->W * d->C;
    const long long We = d->space == SRX_SCORES_Y ? row_in / 3 : d->W;
    if (d->H < 11 || We < 11) return fail(SRX_ERR_BAD_ARG, "%s: H %d and the effective width %lld must be at least 11 (11x11 windows)", who, d->H, We);
    if (row_in > kScoresMaxRow || d->H > kScoresMaxRow)
        return fail(SRX_ERR_BAD_ARG, "%s: sizes overflow: H %d or a row of W*C = %lld floats exceeds %lld", who, d->H, row_in, kScoresMaxRow);
    const int Ce = d->space == SRX_SCORES_Y ? 1 : d->C;
    if (Ce > kScoresMaxCe)
        return fail(SRX_ERR_UNSUPPORTED, "%s: C %d in the rgb space is above %d (the halo of 10 C columns must fit the LDS)", who, d->C, SRX_SCORES_MAX_TAP_STRIDE);
    const long long RL = We * Ce;
    const long long tiles_y = ((long long)d->H - 10 + kScoresTileH - 1) / kScoresTileH, tiles_x = (RL - 10 * Ce + kScoresTileW - 1) / kScoresTileW;
    if (tiles_y * tiles_x > 0x7fffffffLL) return fail(SRX_ERR_BAD_ARG, "%s: sizes overflow: %lld x %lld tiles per image exceed the grid limit", who, tiles_y, tiles_x);
    p->RL = (int)RL; p->Ce = Ce; p->tiles_y = (int)tiles_y; p->tiles_x = (int)tiles_x;
    return SRX_OK;
}

int srx_image_scores_plan(const srx_scores_desc* d, int* tile_h, int* tile_w, int* tiles_y, int* tiles_x) {
    if (!tile_h || !tile_w || !tiles_y || !tiles_x) return fail(SRX_ERR_BAD_ARG, "image_scores_plan: null pointer");
    ScoresPlan p;
    if (int rc = image_scores_plan("image_scores_plan", d, &p)) return rc;
    *tile_h = kScoresTileH; *tile_w = kScoresTileW; *tiles_y = p.tiles_y; *tiles_x = p.tiles_x;
    return SRX_OK;
}

size_t srx_image_scores_scratch_bytes(const srx_scores_desc* d) {
    ScoresPlan p;
    if (image_scores_plan("image_scores_scratch_bytes", d, &p) != SRX_OK) return 0;
    return scores_scratch_floats(d->N, d->n_cand, p.tiles_y * p.tiles_x) * sizeof(float);
}

size_t srx_image_scores_lds_bytes(const srx_scores_desc* d) {
    ScoresPlan p;
    if (image_scores_plan("image_scores_lds_bytes", d, &p) != SRX_OK) return 0;
    return (size_t)scores_lds(p.Ce).bytes;
}

int srx_image_scores(const srx_scores_desc* d, const float* ref, const float* const* cand, float* out, void* scratch,
                     srx_stream_t stream) {
    if (!d || !ref || !cand || !out || !scratch) return fail(SRX_ERR_BAD_ARG, "image_scores: null pointer");
    ScoresPlan p;
    if (int rc = image_scores_plan("image_scores", d, &p)) return rc;
    ImageScoresArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < d->n_cand; ++k) {
        if (!cand[k]) return fail(SRX_ERR_BAD_ARG, "image_scores: null pointer (candidate %d)", k);
        a.cand[k] = cand[k];
    }
    if ((((uintptr_t)out) | ((uintptr_t)scratch)) & 3) return fail(SRX_ERR_ALIGN, "image_scores: out and scratch must be 4-byte aligned");
    if (!launch_image_scores) return fail(SRX_ERR_UNSUPPORTED, "image_scores: this build has no image-scores kernel");
    a.ref = ref;
    a.scratch = (float*)scratch;
    a.H = d->H; a.row_in = d->W * d->C;
    a.RL = p.RL; a.Ce = p.Ce;
    a.n_cand = d->n_cand; a.y_space = d->space == SRX_SCORES_Y; a.unit_clip = d->unit_clip;
    a.tiles_y = p.tiles_y; a.tiles_x = p.tiles_x;
    a.c1 = (0.01f * d->max_val) * (0.01f * d->max_val);       // as launch_ssim
    a.c2 = (0.03f * d->max_val) * (0.03f * d->max_val);
    SRX_CHECK_LAUNCH(launch_image_scores(a, d->N, d->max_val, out, (hipStream_t)stream), "image_scores");
}

// The checks srx_dihedral_expand and srx_dihedral_merge share: the sizes, C, the grid limit and the 4-byte alignment of
// the three pointers (nulls and aliases are the callers': they name the arguments).  `who` prefixes the message.
static int dihedral_check(const char* who, const void* p0, const void* p1, const void* p2, int N, int H, int W, int C) {
    if (N < 1 || H < 1 || W < 1) return fail(SRX_ERR_BAD_ARG, "%s: N %d, H %d and W %d must be at least 1", who, N, H, W);
    if (C < 1 || C > kDihedralMaxC) return fail(SRX_ERR_BAD_ARG, "%s: C %d outside 1..%d", who, C, kDihedralMaxC);
    if ((((uintptr_t)p0) | ((uintptr_t)p1) | ((uintptr_t)p2)) & 3) return fail(SRX_ERR_ALIGN, "%s: pointers must be 4-byte aligned", who);
    if (dihedral_grid(N, H, W).blocks < 0)
        return fail(SRX_ERR_BAD_ARG, "%s: sizes overflow: N %d images of %d x %d pixels are more than %lld tiles of 32 x 32", who, N, H, W,
                    kDihedralMaxTiles);
    return SRX_OK;
}

int srx_dihedral_expand(const float* x, float* a, float* b, int N, int H, int W, int C, srx_stream_t stream) {
    if (!x || !a || !b) return fail(SRX_ERR_BAD_ARG, "dihedral_expand: null pointer");
    if (a == x || b == x || a == b) return fail(SRX_ERR_BAD_ARG, "dihedral_expand: x, a and b must be distinct buffers (not in place)");
    if (int rc = dihedral_check("dihedral_expand", x, a, b, N, H, W, C)) return rc;
    if (!launch_dihedral_expand) return fail(SRX_ERR_UNSUPPORTED, "dihedral_expand: this build has no dihedral kernels");
    SRX_CHECK_LAUNCH(launch_dihedral_expand(x, a, b, N, H, W, C, (hipStream_t)stream), "dihedral_expand");
}

int srx_dihedral_merge(const float* a, const float* b, float* out, int N, int H, int W, int C, srx_stream_t stream) {
    if (!a || !b || !out) return fail(SRX_ERR_BAD_ARG, "dihedral_merge: null pointer");
    if (out == a || out == b) return fail(SRX_ERR_BAD_ARG, "dihedral_merge: out must not be a or b (not in place)");
    if (int rc = dihedral_check("dihedral_merge", a, b, out, N, H, W, C)) return rc;
    if (!launch_dihedral_merge) return fail(SRX_ERR_UNSUPPORTED, "dihedral_merge: this build has no dihedral kernels");
    SRX_CHECK_LAUNCH(launch_dihedral_merge(a, b, out, N, H, W, C, (hipStream_t)stream), "dihedral_merge");
}

int srx_saturate_u8(const float* x, uint8_t* out, size_t numel, srx_stream_t stream) {
    if (!x || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_saturate_u8(x, out, numel, (hipStream_t)stream), "saturate_u8");
}

int srx_affine(const float* x, float* out, size_t numel, float a, float b, srx_stream_t stream) {
    if (!x || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_affine(x, out, numel, a, b, (hipStream_t)stream), "affine");
}

int srx_u8_to_unit_float(const uint8_t* in, float* out, size_t numel, srx_stream_t stream) {
    if (!in || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_u8_to_float(in, out, numel, (hipStream_t)stream), "u8_to_unit_float");
}

int srx_gaussian_blur(const float* in, float* out, float* tmp, int N, int H, int W, int C, float sigma,
                      srx_stream_t stream) {
    if (!in || !out || !tmp) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(SRX_ERR_BAD_ARG, "bad blur dims");
    if (in == out || tmp == in || tmp == out) return fail(SRX_ERR_BAD_ARG, "gaussian blur buffers must be distinct");
    if (sigma > 15.0f) return fail(SRX_ERR_UNSUPPORTED, "sigma %g: radius above 63 not supported", sigma);
    SRX_CHECK_LAUNCH(launch_gaussian_blur(in, out, tmp, N, H, W, C, sigma, (hipStream_t)stream), "gaussian_blur");
}

int srx_resize_bilinear(const float* in, float* out, int N, int H, int W, int C, int OH, int OW, srx_stream_t stream) {
    if (!in || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || OH <= 0 || OW <= 0) return fail(SRX_ERR_BAD_ARG, "bad resize dims");
    SRX_CHECK_LAUNCH(launch_resize_bilinear(in, out, N, H, W, C, OH, OW, (hipStream_t)stream), "resize_bilinear");
}

int srx_upsample_nearest(const float* in, float* out, int N, int H, int W, int C, int f, srx_stream_t stream) {
    if (!in || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || f <= 0) return fail(SRX_ERR_BAD_ARG, "bad upsample dims");
    SRX_CHECK_LAUNCH(launch_upsample_nearest(in, out, N, H, W, C, f, (hipStream_t)stream), "upsample");
}

int srx_upsample_nearest_bwd(const float* dout, float* din, int N, int H, int W, int C, int f, srx_stream_t stream) {
    if (!dout || !din) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || f <= 0) return fail(SRX_ERR_BAD_ARG, "bad upsample dims");
    SRX_CHECK_LAUNCH(launch_upsample_nearest_bwd(dout, din, N, H, W, C, f, (hipStream_t)stream), "upsample_bwd");
}

int srx_debug_poison_lds(srx_stream_t stream) {
    hipError_t err = launch_poison_lds((hipStream_t)stream);
    if (err != hipSuccess) return fail(SRX_ERR_LAUNCH, "poison_lds launch failed: %s", hipGetErrorString(err));
    return SRX_OK;
}

int srx_add_relu_grad(const float* a, const float* b, const float* y, float* out, size_t numel, srx_stream_t stream) {
    if (!a || !b || !y || !out) return fail(SRX_ERR_BAD_ARG, "null pointer");
    if (numel == 0) return SRX_OK;
    SRX_CHECK_LAUNCH(launch_add_relu_grad(a, b, y, out, numel, (hipStream_t)stream), "add_relu_grad");
}

}  // extern "C"
