// pairs_api.hip -- the host side of the eight pair builders (include/srx.h): the four samplers srx_*_patch_pairs and the
// four whole-image builders srx_*_eval_pairs, each with its table check, its walk, its footprint and its entry point.
// What the host and the kernels must agree on is in patch_pairs.h.  No convolution plan is touched here: srx_api.hip keeps
// the planning and routing, the elementwise entry points and the scores.  No device synchronisation, no allocation.
#include <math.h>
#include <stdlib.h>

#include "../../include/srx.h"
#include "patch_pairs.h"

using namespace srx;

namespace srx {
int set_error(int code, const char* fmt, ...);      // srx_api.hip: sets the message srx_last_error returns
}  // namespace srx

namespace {
int (&fail)(int, const char*, ...) = srx::set_error;
}  // namespace
// a launcher's status as the entry point's return code; `what` is the text in front of the runtime's own
#define SRX_CHECK_LAUNCH(expr, what) \
    do { hipError_t e_ = (expr); return e_ == hipSuccess ? SRX_OK : fail(SRX_ERR_LAUNCH, what ": %s", hipGetErrorString(e_)); } while (0)

extern "C" {

// resample_u8.hip's host routines, which srx_enet_pairs_tables builds its block with: weak references, like the launchers
// of patch_pairs.h, so that a host-only build of this unit links without them, and srx_enet_pairs_tables refuses.
__attribute__((weak)) int srx_pil_resample_ksize(int in_size, int out_size, int filter);
__attribute__((weak)) int srx_pil_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk);

// Entry e's width x height x 3 bytes at `offset` lie inside the arena: the only thing between a host table and a kernel's
// global reads, for the four samplers (patch_entry_geometry) and the four whole-image builders (the eval walks) alike.
// width, height < 2^31: the product fits 64 bits; the sum with the offset is never formed.
static int image_inside_arena(const char* who, int e, uint64_t offset, int width, int height, size_t arena_bytes) {
    const uint64_t bytes = (uint64_t)width * (uint64_t)height * 3u;
    if (bytes > (uint64_t)arena_bytes || offset > (uint64_t)arena_bytes - bytes)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %llu bytes at offset %llu leaves the arena of %zu bytes", who, e,
                    (unsigned long long)bytes, (unsigned long long)offset, arena_bytes);
    return SRX_OK;
}

// The geometry every sampler's table check enforces on entry e: the image has pixels, the `side` x `side` window (`noun`:
// "crop" or "patch") lies inside the image, and the image lies inside the arena.  `who` prefixes the message.
static_assert(sizeof(srx_patch_src) == 32, "srx_patch_src is 32 bytes (include/srx.h)");
static int patch_entry_geometry(const char* who, int e, const srx_patch_src& t, int side, const char* noun, size_t arena_bytes) {
    if (t.width < 1 || t.height < 1) return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels", who, e, t.width, t.height);
    if (t.x < 0 || t.y < 0 || (int64_t)t.x + side > t.width || (int64_t)t.y + side > t.height)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %s of %d at x %d y %d leaves its %d x %d image", who, e, noun, side, t.x, t.y,
                    t.width, t.height);
    return image_inside_arena(who, e, t.offset, t.width, t.height, arena_bytes);
}

int srx_vdsr_patch_table_check(const srx_patch_src* table_host, int B, int S, size_t arena_bytes) {
    if (!table_host) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: null table");
    if (B < 1 || B > kPatchMaxB) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: B %d outside 1..%d", B, kPatchMaxB);
    if (S < kPatchMinS || S > kPatchMaxS)
        return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: S %d outside %d..%d", S, kPatchMinS, kPatchMaxS);
    for (int e = 0; e < B; ++e) {
        const srx_patch_src& t = table_host[e];
        if (int rc = patch_entry_geometry("vdsr_patch_table_check", e, t, S, "crop", arena_bytes)) return rc;
        if (t.flip != 0 && t.flip != 1) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: entry %d: flip %d is not 0 or 1", e, t.flip);
        const float f = t.scaling_factor;
        if (!isfinite(f) || !(f > 1.0f))
            return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: entry %d: scaling factor %g is not a finite number above 1", e, (double)f);
        if (patch_lr_size(S, f) < 1)
            return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: entry %d: int(S / factor) = int(%d / %g) is below 1", e, S, (double)f);
        if (patch_radius(f) > kPatchMaxRadius)
            return fail(SRX_ERR_BAD_ARG, "vdsr_patch_table_check: entry %d: factor %g gives a blur radius of %d, above %d", e, (double)f,
                        patch_radius(f), kPatchMaxRadius);
    }
    return SRX_OK;
}

int srx_vdsr_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S, float* sd, float* hd,
                         srx_stream_t stream) {
    if (!arena || !table_dev || !sd || !hd) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_pairs: null pointer");
    if (B < 1 || B > kPatchMaxB) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_pairs: B %d outside 1..%d", B, kPatchMaxB);
    if (S < kPatchMinS || S > kPatchMaxS) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_pairs: S %d outside %d..%d", S, kPatchMinS, kPatchMaxS);
    if (sd == hd) return fail(SRX_ERR_BAD_ARG, "vdsr_patch_pairs: sd and hd must be distinct");
    if (!launch_vdsr_patch_pairs) return fail(SRX_ERR_UNSUPPORTED, "vdsr_patch_pairs: this build has no patch-pair kernel");
    const PatchPairsArgs a = {arena, table_dev, sd, hd, S};
    SRX_CHECK_LAUNCH(launch_vdsr_patch_pairs(a, B, (hipStream_t)stream), "vdsr_patch_pairs");
}

// r, p limits shared by the check and the entry point; `who` prefixes the message
static int espcn_pairs_limits(const char* who, int r, int p) {
    if (r < kEspcnMinR || r > kEspcnMaxR) return fail(SRX_ERR_BAD_ARG, "%s: r %d outside %d..%d", who, r, kEspcnMinR, kEspcnMaxR);
    if (p < 1 || p > kEspcnMaxP / r) return fail(SRX_ERR_BAD_ARG, "%s: p %d outside 1..%d (p * r <= %d)", who, p, kEspcnMaxP / r, kEspcnMaxP);
    return SRX_OK;
}

int srx_espcn_patch_table_check(const srx_patch_src* table_host, int n, int r, int p, size_t arena_bytes) {
    if (!table_host) return fail(SRX_ERR_BAD_ARG, "espcn_patch_table_check: null table");
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "espcn_patch_table_check: n %d below 1", n);
    if (int rc = espcn_pairs_limits("espcn_patch_table_check", r, p)) return rc;
    const int P = p * r;
    for (int e = 0; e < n; ++e) {
        const srx_patch_src& t = table_host[e];
        if (int rc = patch_entry_geometry("espcn_patch_table_check", e, t, P, "patch", arena_bytes)) return rc;
        if (t.flip < 0 || t.flip > 3) return fail(SRX_ERR_BAD_ARG, "espcn_patch_table_check: entry %d: flip %d outside 0..3", e, t.flip);
        if (!(t.scaling_factor == (float)r))
            return fail(SRX_ERR_BAD_ARG, "espcn_patch_table_check: entry %d: scaling factor %g is not the table's r %d", e,
                        (double)t.scaling_factor, r);
    }
    return SRX_OK;
}

int srx_espcn_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int r, int p, float* lr, float* label,
                          srx_stream_t stream) {
    if (!arena || !table_dev || !lr || !label) return fail(SRX_ERR_BAD_ARG, "espcn_patch_pairs: null pointer");
    if (B < 1) return fail(SRX_ERR_BAD_ARG, "espcn_patch_pairs: B %d below 1", B);
    if (int rc = espcn_pairs_limits("espcn_patch_pairs", r, p)) return rc;
    if (lr == label) return fail(SRX_ERR_BAD_ARG, "espcn_patch_pairs: lr and label must be distinct");
    if (!launch_espcn_patch_pairs) return fail(SRX_ERR_UNSUPPORTED, "espcn_patch_pairs: this build has no patch-pair kernel");
    const EspcnPairsArgs a = {arena, table_dev, lr, label, r, p};
    SRX_CHECK_LAUNCH(launch_espcn_patch_pairs(a, B, (hipStream_t)stream), "espcn_patch_pairs");
}

// What the four whole-image walks below ask in the same words: a table and entries to walk, a first_tile that continues
// the running sum of tiles, (own < 2^54: no overflow) a running sum that stays at or below kEvalMaxTiles, and -- the two
// walks with two outputs, EnhanceNet's and SRCNN's -- running sums of floats padded to 4.
static int eval_table_args(const char* who, const void* table, int n) {
    if (!table) return fail(SRX_ERR_BAD_ARG, "%s: null table", who);
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "%s: n %d below 1", who, n);
    return SRX_OK;
}
static int eval_first_tile(const char* who, int e, uint32_t first_tile, uint64_t tiles) {
    if ((uint64_t)first_tile != tiles)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: first_tile %u is not the %llu tiles of the entries before it", who, e, first_tile,
                    (unsigned long long)tiles);
    return SRX_OK;
}
static int eval_add_tiles(const char* who, int e, uint64_t own, uint64_t* tiles) {
    *tiles += own;
    if (*tiles > kEvalMaxTiles)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %llu tiles up to this entry, above %llu", who, e, (unsigned long long)*tiles,
                    (unsigned long long)kEvalMaxTiles);
    return SRX_OK;
}
// Entry e's K outputs (`names`: their offset fields) in K running sums: offsets[k] is start[k], where the entry must begin
// (the end of the one before it, padded to 4 floats); its own[k] floats fit the output's totals[k]; then end[k] is where it
// ends and start[k] where the next begins.  own < 2^50: no sum here overflows.  vdsr_eval_walk words its one sum
// differently (it names out_floats) and keeps its own lines; ESPCN's lr_offset is not padded.
static int eval_padded_sums(const char* who, int e, int K, const char* const* names, const uint64_t* offsets, const uint64_t* own,
                            const uint64_t* totals, uint64_t* start, uint64_t* end) {
    for (int k = 0; k < K; ++k) {
        if (offsets[k] != start[k])
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %s %llu is not %llu, the floats of the entries before it padded to 4", who, e,
                        names[k], (unsigned long long)offsets[k], (unsigned long long)start[k]);
        if (start[k] > totals[k] || own[k] > totals[k] - start[k])
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %llu floats from %s %llu on are more than the output's %llu", who, e,
                        (unsigned long long)own[k], names[k], (unsigned long long)start[k], (unsigned long long)totals[k]);
        end[k] = start[k] + own[k];
        start[k] = eval_padded(end[k]);
    }
    return SRX_OK;
}

// The walk srx_espcn_eval_table_check and srx_espcn_eval_tiles share: the table's arguments, every entry's sizes and the tile
// count, which never passes kEvalMaxTiles (so no sum here overflows).  With `bounds` = {arena_bytes, lr_floats} (the
// check) every entry is also held to the arena, to reserved == 0 and to the running sums of lr floats and tiles, and the
// total to lr_floats; null (the tile count) skips that.  `who` prefixes the message.
static_assert(sizeof(srx_eval_image) == 32, "srx_eval_image is 32 bytes (include/srx.h)");
static int espcn_eval_walk(const char* who, const srx_eval_image* table, int n, int r, const size_t* bounds, uint64_t* tiles_out) {
    if (int rc = eval_table_args(who, table, n)) return rc;
    if (r < kEspcnMinR || r > kEspcnMaxR) return fail(SRX_ERR_BAD_ARG, "%s: r %d outside %d..%d", who, r, kEspcnMinR, kEspcnMaxR);
    uint64_t tiles = 0, floats = 0;      // floats: the running sum of lr floats, never above lr_floats
    for (int e = 0; e < n; ++e) {
        const srx_eval_image& t = table[e];
        if (t.width < r || t.height < r || t.width % r || t.height % r)
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels: each side must be a multiple of r %d, at least r", who, e,
                        t.width, t.height, r);
        if (bounds) {
            const size_t arena_bytes = bounds[0], lr_floats = bounds[1];
            if (int rc = image_inside_arena(who, e, t.offset, t.width, t.height, arena_bytes)) return rc;
            if (t.reserved != 0) return fail(SRX_ERR_BAD_ARG, "%s: entry %d: reserved %u is not 0", who, e, t.reserved);
            if (t.lr_offset != floats)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: lr_offset %llu is not the %llu lr floats of the entries before it", who, e,
                            (unsigned long long)t.lr_offset, (unsigned long long)floats);
            if (int rc = eval_first_tile(who, e, t.first_tile, tiles)) return rc;
            const uint64_t own = (uint64_t)(t.height / r) * (uint64_t)(t.width / r) * 3u;      // below 2^62
            if (own > (uint64_t)lr_floats - floats)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %llu lr floats after %llu before it are more than lr_floats %zu", who, e,
                            (unsigned long long)own, (unsigned long long)floats, lr_floats);
            floats += own;
        }
        if (int rc = eval_add_tiles(who, e, eval_image_tiles(t.width / r, t.height / r, espcn_eval_tile()), &tiles)) return rc;
    }
    if (bounds && floats != (uint64_t)bounds[1])
        return fail(SRX_ERR_BAD_ARG, "%s: the table's %d entries hold %llu lr floats, not lr_floats %zu", who, n, (unsigned long long)floats,
                    bounds[1]);
    *tiles_out = tiles;
    return SRX_OK;
}

int srx_espcn_eval_table_check(const srx_eval_image* table_host, int n, int r, size_t arena_bytes, size_t lr_floats) {
    const size_t bounds[2] = {arena_bytes, lr_floats};
    uint64_t tiles = 0;
    return espcn_eval_walk("espcn_eval_table_check", table_host, n, r, bounds, &tiles);
}

size_t srx_espcn_eval_tiles(const srx_eval_image* table_host, int n, int r) {
    uint64_t tiles = 0;
    if (espcn_eval_walk("espcn_eval_tiles", table_host, n, r, nullptr, &tiles)) return 0;
    return (size_t)tiles;
}

int srx_espcn_eval_pairs(const uint8_t* arena, const srx_eval_image* table_dev, int n, int r, float* lr, float* label,
                         srx_stream_t stream) {
    if (!arena || !table_dev || !lr || !label) return fail(SRX_ERR_BAD_ARG, "espcn_eval_pairs: null pointer");
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "espcn_eval_pairs: n %d below 1", n);
    if (r < kEspcnMinR || r > kEspcnMaxR) return fail(SRX_ERR_BAD_ARG, "espcn_eval_pairs: r %d outside %d..%d", r, kEspcnMinR, kEspcnMaxR);
    if (lr == label) return fail(SRX_ERR_BAD_ARG, "espcn_eval_pairs: lr and label must be distinct");
    if (!launch_espcn_eval_pairs) return fail(SRX_ERR_UNSUPPORTED, "espcn_eval_pairs: this build has no eval-pair kernel");
    const EspcnEvalArgs a = {arena, table_dev, lr, label, n, r};
    SRX_CHECK_LAUNCH(launch_espcn_eval_pairs(a, (hipStream_t)stream), "espcn_eval_pairs");
}

// One axis of a record for srx_vdsr_eval_table_check: the largest n_src, n_samp and n_lo over its tiles (patch_pairs.h:
// vdsr_eval_axis), and that every tile's ranges are ordered and inside the image -- which the monotone taps guarantee, and
// which is what the kernel's reads rely on.  O(side / T).
struct VdsrEvalAxisMax {
    int n_src, n_samp, n_lo;
    bool sane;
};
static VdsrEvalAxisMax vdsr_eval_axis_max(int side, float s) {
    const int L = patch_lr_size(side, s), R = patch_radius(s), tiles = eval_tiles_along(side, SRX_VDSR_EVAL_TILE);
    VdsrEvalAxisMax m = {0, 0, 0, true};
    for (int k = 0; k < tiles; ++k) {
        const VdsrEvalAxis a = vdsr_eval_axis(side, L, R, k);
        m.n_src = a.n_src > m.n_src ? a.n_src : m.n_src;
        m.n_samp = a.n_samp > m.n_samp ? a.n_samp : m.n_samp;
        m.n_lo = a.n_lo > m.n_lo ? a.n_lo : m.n_lo;
        m.sane = m.sane && 0 <= a.lo_first && a.lo_first <= a.lo_last && a.lo_last < L && 0 <= a.bl_first && a.bl_first <= a.bl_last &&
                 a.bl_last < side && 0 <= a.src_first && a.src_first <= a.bl_first && a.bl_last <= a.src_last && a.src_last < side;
    }
    return m;
}

// What srx_vdsr_eval_table_check, srx_vdsr_eval_tiles and srx_vdsr_eval_footprint ask of a side and a factor
static bool vdsr_eval_factor_and_sizes_ok(int width, int height, float s) {
    return vdsr_eval_factor_ok(s) && patch_lr_size(height, s) >= 1 && patch_lr_size(width, s) >= 1;
}

// The walk srx_vdsr_eval_table_check and srx_vdsr_eval_tiles share, as espcn_eval_walk: the table's arguments, every entry's
// sizes and the tile count, which never passes kEvalMaxTiles.  With `bounds` = {arena_bytes, out_floats} (the check)
// every entry is also held to its factor, the arena, the running sums, the LDS layout, and the total to out_floats.
static_assert(sizeof(srx_vdsr_eval_image) == 32, "srx_vdsr_eval_image is 32 bytes (include/srx.h)");
static int vdsr_eval_walk(const char* who, const srx_vdsr_eval_image* table, int n, const size_t* bounds, uint64_t* tiles_out) {
    if (int rc = eval_table_args(who, table, n)) return rc;
    uint64_t tiles = 0, start = 0, end = 0;      // start: where this entry must begin (padded); end: where the one before it ends
    for (int e = 0; e < n; ++e) {
        const srx_vdsr_eval_image& t = table[e];
        if (t.width < 1 || t.height < 1)
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels: each side must be at least 1", who, e, t.width, t.height);
        if (bounds) {
            const size_t arena_bytes = bounds[0], out_floats = bounds[1];
            const float s = t.scaling_factor;
            if (!vdsr_eval_factor_ok(s))
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: scaling_factor %g is not a finite value in (1, %g]", who, e, (double)s,
                            (double)kVdsrEvalMaxS);
            if (!vdsr_eval_factor_and_sizes_ok(t.width, t.height, s))
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels has no low-resolution pixel at scaling_factor %g", who,
                            e, t.width, t.height, (double)s);
            if (int rc = image_inside_arena(who, e, t.offset, t.width, t.height, arena_bytes)) return rc;
            if (t.out_offset != start)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: out_offset %llu is not %llu, the floats of the entries before it padded to 4",
                            who, e, (unsigned long long)t.out_offset, (unsigned long long)start);
            if (int rc = eval_first_tile(who, e, t.first_tile, tiles)) return rc;
            const uint64_t own = eval_image_floats(t.width, t.height);      // below 2^64 / 5; start <= out_floats here
            if (start > (uint64_t)out_floats || own > (uint64_t)out_floats - start)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: %llu floats from %llu on are more than out_floats %zu", who, e,
                            (unsigned long long)own, (unsigned long long)start, out_floats);
            end = start + own;
            start = eval_padded(end);
            const VdsrEvalAxisMax my = vdsr_eval_axis_max(t.height, s), mx = vdsr_eval_axis_max(t.width, s);
            const int need = vdsr_eval_lds(my.n_src, mx.n_src, my.n_samp, my.n_lo, mx.n_lo).bytes;
            if (!my.sane || !mx.sane || patch_radius(s) > kVdsrEvalMaxRadius || need > kVdsrEvalLdsBytes)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: a tile's footprint (%d x %d source pixels, %d sampled rows, %d x %d "
                            "low-resolution pixels: %d bytes) is beyond the LDS layout of %d bytes", who, e, my.n_src, mx.n_src, my.n_samp,
                            my.n_lo, mx.n_lo, need, kVdsrEvalLdsBytes);
        }
        if (int rc = eval_add_tiles(who, e, eval_image_tiles(t.width, t.height, SRX_VDSR_EVAL_TILE), &tiles)) return rc;
    }
    if (bounds && end != (uint64_t)bounds[1])
        return fail(SRX_ERR_BAD_ARG, "%s: the table's %d entries end at float %llu, not at out_floats %zu", who, n, (unsigned long long)end,
                    bounds[1]);
    *tiles_out = tiles;
    return SRX_OK;
}

int srx_vdsr_eval_table_check(const srx_vdsr_eval_image* table_host, int n, size_t arena_bytes, size_t out_floats) {
    const size_t bounds[2] = {arena_bytes, out_floats};
    uint64_t tiles = 0;
    return vdsr_eval_walk("vdsr_eval_table_check", table_host, n, bounds, &tiles);
}

size_t srx_vdsr_eval_tiles(const srx_vdsr_eval_image* table_host, int n) {
    uint64_t tiles = 0;
    if (vdsr_eval_walk("vdsr_eval_tiles", table_host, n, nullptr, &tiles)) return 0;
    return (size_t)tiles;
}

int srx_vdsr_eval_footprint(int side, float s, int tile, int out[6]) {
    if (!out) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_footprint: null out");
    if (side < 1) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_footprint: side %d below 1", side);
    if (!vdsr_eval_factor_ok(s)) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_footprint: s %g is not a finite value in (1, %g]", (double)s, (double)kVdsrEvalMaxS);
    const int L = patch_lr_size(side, s);
    if (L < 1) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_footprint: a side of %d pixels has no low-resolution pixel at s %g", side, (double)s);
    if (tile < 0 || tile >= eval_tiles_along(side, SRX_VDSR_EVAL_TILE))
        return fail(SRX_ERR_BAD_ARG, "vdsr_eval_footprint: tile %d outside 0..%d", tile, eval_tiles_along(side, SRX_VDSR_EVAL_TILE) - 1);
    const VdsrEvalAxis a = vdsr_eval_axis(side, L, patch_radius(s), tile);
    out[0] = a.lo_first; out[1] = a.lo_last; out[2] = a.bl_first; out[3] = a.bl_last; out[4] = a.src_first; out[5] = a.src_last;
    return SRX_OK;
}

int srx_vdsr_eval_pairs(const uint8_t* arena, const srx_vdsr_eval_image* table_dev, int n, float* sd, float* hd, srx_stream_t stream) {
    if (!arena || !table_dev || !sd || !hd) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_pairs: null pointer");
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_pairs: n %d below 1", n);
    if (sd == hd) return fail(SRX_ERR_BAD_ARG, "vdsr_eval_pairs: sd and hd must be distinct");
    if (!launch_vdsr_eval_pairs) return fail(SRX_ERR_UNSUPPORTED, "vdsr_eval_pairs: this build has no eval-pair kernel");
    const VdsrEvalArgs a = {arena, table_dev, sd, hd, n};
    SRX_CHECK_LAUNCH(launch_vdsr_eval_pairs(a, (hipStream_t)stream), "vdsr_eval_pairs");
}

// S limits shared by the four entry points; `who` prefixes the message
static int enet_pairs_limits(const char* who, int S) {
    if (!enet_pairs_size_ok(S)) return fail(SRX_ERR_BAD_ARG, "%s: S %d is not a multiple of 4 in %d..%d", who, S, kEnetMinS, kEnetMaxS);
    return SRX_OK;
}

int srx_enet_pairs_table_words(int S) {
    if (enet_pairs_limits("enet_pairs_table_words", S)) return -1;
    return enet_pairs_tables(S).words;
}

// The block of enet_pairs_tables(S) for a multiple of 4, S >= 4, written at words_host: what srx_enet_pairs_tables and
// srx_enet_eval_coeffs share.  `who` prefixes the message.
static int enet_write_tables(const char* who, int S, int32_t* words_host) {
    if (!srx_pil_resample_ksize || !srx_pil_resample_coeffs) return fail(SRX_ERR_UNSUPPORTED, "%s: this build has no resample unit", who);
    const int s = S / 4;
    // the block's layout fixes the window sizes (patch_pairs.h); they are Pillow's for the ratio 4 at every S
    if (srx_pil_resample_ksize(S, s, SRX_RESAMPLE_BILINEAR) != kEnetKDown || srx_pil_resample_ksize(s, S, SRX_RESAMPLE_BICUBIC) != kEnetKUp)
        return fail(SRX_ERR_UNSUPPORTED, "%s: S %d: window sizes are not %d and %d", who, S, kEnetKDown, kEnetKUp);
    const EnetPairsTables t = enet_pairs_tables(S);
    if (int rc = srx_pil_resample_coeffs(S, s, SRX_RESAMPLE_BILINEAR, words_host + t.down_bounds, words_host + t.down_kk)) return rc;
    return srx_pil_resample_coeffs(s, S, SRX_RESAMPLE_BICUBIC, words_host + t.up_bounds, words_host + t.up_kk);
}

int srx_enet_pairs_tables(int S, int32_t* words_host) {
    if (int rc = enet_pairs_limits("enet_pairs_tables", S)) return rc;
    if (!words_host) return fail(SRX_ERR_BAD_ARG, "enet_pairs_tables: null block");
    return enet_write_tables("enet_pairs_tables", S, words_host);
}

int srx_enet_patch_table_check(const srx_patch_src* table_host, int B, int S, size_t arena_bytes) {
    if (!table_host) return fail(SRX_ERR_BAD_ARG, "enet_patch_table_check: null table");
    if (B < 1) return fail(SRX_ERR_BAD_ARG, "enet_patch_table_check: B %d below 1", B);
    if (int rc = enet_pairs_limits("enet_patch_table_check", S)) return rc;
    for (int e = 0; e < B; ++e) {
        const srx_patch_src& t = table_host[e];
        if (int rc = patch_entry_geometry("enet_patch_table_check", e, t, S, "crop", arena_bytes)) return rc;
        if (t.flip < 0 || t.flip > 3) return fail(SRX_ERR_BAD_ARG, "enet_patch_table_check: entry %d: flip %d outside 0..3", e, t.flip);
        if (!(t.scaling_factor == 4.0f))
            return fail(SRX_ERR_BAD_ARG, "enet_patch_table_check: entry %d: scaling factor %g is not 4", e, (double)t.scaling_factor);
    }
    return SRX_OK;
}

int srx_enet_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S, const int32_t* tables_dev, float* sd,
                         float* bq, float* hd, srx_stream_t stream) {
    if (!arena || !table_dev || !tables_dev || !sd || !bq || !hd) return fail(SRX_ERR_BAD_ARG, "enet_patch_pairs: null pointer");
    if (B < 1) return fail(SRX_ERR_BAD_ARG, "enet_patch_pairs: B %d below 1", B);
    if (int rc = enet_pairs_limits("enet_patch_pairs", S)) return rc;
    if (sd == bq || sd == hd || bq == hd) return fail(SRX_ERR_BAD_ARG, "enet_patch_pairs: sd, bq and hd must be distinct");
    if (!launch_enet_patch_pairs) return fail(SRX_ERR_UNSUPPORTED, "enet_patch_pairs: this build has no patch-pair kernel");
    const EnetPairsArgs a = {arena, table_dev, tables_dev, sd, bq, hd, S};
    SRX_CHECK_LAUNCH(launch_enet_patch_pairs(a, B, (hipStream_t)stream), "enet_patch_pairs");
}

// ---- EnhanceNet's whole-image pairs (enet/enet/datasets.py:95-127; enet_eval.hip) ----

int srx_enet_eval_coeff_words(int side) {
    if (side < kEnetMinS || side > kEnetEvalMaxSide || (side & 3))
        return fail(SRX_ERR_BAD_ARG, "enet_eval_coeff_words: side %d is not a multiple of 4 in %d..%d", side, kEnetMinS, kEnetEvalMaxSide), -1;
    return enet_eval_block_words(side);
}

int srx_enet_eval_coeffs(int side, int32_t* out) {
    if (side < kEnetMinS || side > kEnetEvalMaxSide || (side & 3))
        return fail(SRX_ERR_BAD_ARG, "enet_eval_coeffs: side %d is not a multiple of 4 in %d..%d", side, kEnetMinS, kEnetEvalMaxSide);
    if (!out) return fail(SRX_ERR_BAD_ARG, "enet_eval_coeffs: null block");
    out[0] = side;      // what srx_enet_eval_table_check compares with a record's side
    return enet_write_tables("enet_eval_coeffs", side, out + kEnetEvalBlockHeader);
}

// bounds [out][2] = (first, count) of a resample from `in` pixels with `ksize` taps are Pillow's in shape: every output
// has 1..ksize taps inside the input, and neither the first index nor the end decreases -- what lets enet_eval_axis take a
// run's reach from its two ends, and what keeps every tap of the kernel's passes inside the footprint.
static bool enet_eval_bounds_sane(const int32_t* bounds, int out, int in, int ksize) {
    int first_before = 0, end_before = 0;
    for (int o = 0; o < out; ++o) {
        const int first = bounds[2 * o], count = bounds[2 * o + 1];
        if (count < 1 || count > ksize || first < 0 || first > in - count) return false;
        if (first < first_before || first + count < end_before) return false;
        first_before = first;
        end_before = first + count;
    }
    return true;
}

// One axis of a record for srx_enet_eval_table_check: the largest n_hd, n_sd and n_out over its tiles (patch_pairs.h:
// enet_eval_axis), and that every tile's footprint is ordered, inside the image and around the tile's own pixels -- which
// is what the kernel's reads rely on.  `tables`: the axis's block past its header, its bounds already found sane.
struct EnetEvalAxisMax {
    int n_hd, n_sd, n_out;
    bool sane;
};
static EnetEvalAxisMax enet_eval_axis_max(const int32_t* tables, int side) {
    EnetEvalAxisMax m = {0, 0, 0, true};
    for (int k = 0; k < eval_tiles_along(side, SRX_ENET_EVAL_TILE); ++k) {
        const EnetEvalAxis a = enet_eval_axis(tables, side, k);
        m.n_hd = a.n_hd > m.n_hd ? a.n_hd : m.n_hd;
        m.n_sd = a.n_sd > m.n_sd ? a.n_sd : m.n_sd;
        m.n_out = a.n_out > m.n_out ? a.n_out : m.n_out;
        m.sane = m.sane && 0 <= a.sd_first && a.sd_first <= a.own_first && a.own_last <= a.sd_last && a.sd_last < side / 4 &&
                 0 <= a.hd_first && a.hd_first <= a.out_first && a.out_last <= a.hd_last && a.hd_last < side;
    }
    m.sane = m.sane && m.n_hd <= kEnetEvalMaxReach && m.n_sd <= kEnetEvalMaxReach;
    return m;
}

// What srx_enet_eval_table_check holds a record's two outputs and its coefficient arena to
struct EnetEvalBounds {
    size_t arena_bytes, out_floats, sd_floats;
    const int32_t* coeffs;
    size_t coeff_words;
};

// The block of `side` at word `at` of the coefficient arena: inside it, built for `side` (its first word) and sane.  On
// success *tables is the block past its header.
static int enet_eval_block(const char* who, int e, const char* axis, int side, uint32_t at, const EnetEvalBounds& b, const int32_t** tables) {
    const uint64_t words = (uint64_t)enet_eval_block_words(side);
    if ((uint64_t)at > (uint64_t)b.coeff_words || words > (uint64_t)b.coeff_words - at)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: the %s block of %llu words at word %u leaves the coefficient arena of %zu words", who, e,
                    axis, (unsigned long long)words, at, b.coeff_words);
    const int32_t* block = b.coeffs + at;
    if (block[0] != side)
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: the %s block at word %u was built for a side of %d, not %d", who, e, axis, at, block[0], side);
    const EnetPairsTables t = enet_pairs_tables(side);
    const int32_t* body = block + kEnetEvalBlockHeader;
    if (!enet_eval_bounds_sane(body + t.down_bounds, side / 4, side, kEnetKDown) || !enet_eval_bounds_sane(body + t.up_bounds, side, side / 4, kEnetKUp))
        return fail(SRX_ERR_BAD_ARG, "%s: entry %d: the bounds of the %s block at word %u are not those of a resample of %d pixels", who, e,
                    axis, at, side);
    *tables = body;
    return SRX_OK;
}

// The walk srx_enet_eval_table_check and srx_enet_eval_tiles share, as vdsr_eval_walk: the table's arguments, every entry's
// sides and the tile count, which never passes kEvalMaxTiles.  With `bounds` (the check) every entry is also held to the
// arena, the running sums, its coefficient blocks and the LDS layout, and the totals to out_floats and sd_floats.
static_assert(sizeof(srx_enet_eval_image) == 48, "srx_enet_eval_image is 48 bytes (include/srx.h)");
static_assert(SRX_ENET_EVAL_TILE % 4 == 0 && SRX_ENET_EVAL_TILE >= 4, "a tile holds whole sd pixels");
static int enet_eval_walk(const char* who, const srx_enet_eval_image* table, int n, const EnetEvalBounds* bounds, uint64_t* tiles_out) {
    if (int rc = eval_table_args(who, table, n)) return rc;
    if (bounds && !bounds->coeffs) return fail(SRX_ERR_BAD_ARG, "%s: null coefficient arena", who);
    uint64_t tiles = 0;
    uint64_t start[2] = {0, 0}, end[2] = {0, 0};      // [0]: hd and bq, [1]: sd; start: where this entry must begin (padded)
    for (int e = 0; e < n; ++e) {
        const srx_enet_eval_image& t = table[e];
        if (!enet_eval_side_ok(t.width) || !enet_eval_side_ok(t.height))
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels: each side must be a multiple of 4 in %d..%d", who, e, t.width,
                        t.height, kEnetEvalMinSide, kEnetEvalMaxSide);
        if (bounds) {
            if (int rc = image_inside_arena(who, e, t.offset, t.width, t.height, bounds->arena_bytes)) return rc;
            if (t.reserved != 0) return fail(SRX_ERR_BAD_ARG, "%s: entry %d: reserved %u is not 0", who, e, t.reserved);
            if (int rc = eval_first_tile(who, e, t.first_tile, tiles)) return rc;
            const uint64_t offsets[2] = {t.out_offset, t.sd_offset};
            const uint64_t own[2] = {eval_image_floats(t.width, t.height), eval_image_floats(t.width / 4, t.height / 4)};
            const uint64_t totals[2] = {(uint64_t)bounds->out_floats, (uint64_t)bounds->sd_floats};
            static const char* const names[2] = {"out_offset", "sd_offset"};
            if (int rc = eval_padded_sums(who, e, 2, names, offsets, own, totals, start, end)) return rc;
            const int32_t *tables_x = nullptr, *tables_y = nullptr;
            if (int rc = enet_eval_block(who, e, "width", t.width, t.width_coeffs, *bounds, &tables_x)) return rc;
            if (int rc = enet_eval_block(who, e, "height", t.height, t.height_coeffs, *bounds, &tables_y)) return rc;
            const EnetEvalAxisMax my = enet_eval_axis_max(tables_y, t.height), mx = enet_eval_axis_max(tables_x, t.width);
            const int need = my.sane && mx.sane ? enet_eval_lds(my.n_hd, mx.n_hd, my.n_sd, mx.n_sd, my.n_out, mx.n_out).bytes : 0;
            if (!my.sane || !mx.sane || need > kEnetEvalLdsBytes)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: a tile's footprint (%d x %d hd pixels, %d x %d sd pixels: %d bytes) leaves the "
                            "image or is beyond the LDS layout of %d bytes", who, e, my.n_hd, mx.n_hd, my.n_sd, mx.n_sd, need, kEnetEvalLdsBytes);
        }
        if (int rc = eval_add_tiles(who, e, eval_image_tiles(t.width, t.height, SRX_ENET_EVAL_TILE), &tiles)) return rc;
    }
    if (bounds && (end[0] != (uint64_t)bounds->out_floats || end[1] != (uint64_t)bounds->sd_floats))
        return fail(SRX_ERR_BAD_ARG, "%s: the table's %d entries end at float %llu of hd and %llu of sd, not at out_floats %zu and sd_floats %zu",
                    who, n, (unsigned long long)end[0], (unsigned long long)end[1], bounds->out_floats, bounds->sd_floats);
    *tiles_out = tiles;
    return SRX_OK;
}

int srx_enet_eval_table_check(const srx_enet_eval_image* table_host, int n, size_t arena_bytes, size_t out_floats, size_t sd_floats,
                              const int32_t* coeffs_host, size_t coeff_words) {
    const EnetEvalBounds bounds = {arena_bytes, out_floats, sd_floats, coeffs_host, coeff_words};
    uint64_t tiles = 0;
    return enet_eval_walk("enet_eval_table_check", table_host, n, &bounds, &tiles);
}

size_t srx_enet_eval_tiles(const srx_enet_eval_image* table_host, int n) {
    uint64_t tiles = 0;
    if (enet_eval_walk("enet_eval_tiles", table_host, n, nullptr, &tiles)) return 0;
    return (size_t)tiles;
}

int srx_enet_eval_footprint(int side, int tile, int out[4]) {
    if (!out) return fail(SRX_ERR_BAD_ARG, "enet_eval_footprint: null out");
    if (!enet_eval_side_ok(side))
        return fail(SRX_ERR_BAD_ARG, "enet_eval_footprint: side %d is not a multiple of 4 in %d..%d", side, kEnetEvalMinSide, kEnetEvalMaxSide);
    if (tile < 0 || tile >= eval_tiles_along(side, SRX_ENET_EVAL_TILE))
        return fail(SRX_ERR_BAD_ARG, "enet_eval_footprint: tile %d outside 0..%d", tile, eval_tiles_along(side, SRX_ENET_EVAL_TILE) - 1);
    int32_t* block = (int32_t*)malloc(sizeof(int32_t) * (size_t)enet_eval_block_words(side));
    if (!block) return fail(SRX_ERR_BAD_ARG, "enet_eval_footprint: no memory for the block of side %d", side);
    int rc = srx_enet_eval_coeffs(side, block);
    if (rc == SRX_OK) {
        const EnetEvalAxis a = enet_eval_axis(block + kEnetEvalBlockHeader, side, tile);
        out[0] = a.sd_first; out[1] = a.sd_last; out[2] = a.hd_first; out[3] = a.hd_last;
    }
    free(block);
    return rc;
}

int srx_enet_eval_pairs(const uint8_t* arena, const srx_enet_eval_image* table_dev, int n, const int32_t* coeffs_dev, float* sd, float* bq,
                        float* hd, srx_stream_t stream) {
    if (!arena || !table_dev || !coeffs_dev || !sd || !bq || !hd) return fail(SRX_ERR_BAD_ARG, "enet_eval_pairs: null pointer");
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "enet_eval_pairs: n %d below 1", n);
    if (sd == bq || sd == hd || bq == hd) return fail(SRX_ERR_BAD_ARG, "enet_eval_pairs: sd, bq and hd must be distinct");
    if (!launch_enet_eval_pairs) return fail(SRX_ERR_UNSUPPORTED, "enet_eval_pairs: this build has no eval-pair kernel");
    const EnetEvalArgs a = {arena, table_dev, coeffs_dev, sd, bq, hd, n};
    SRX_CHECK_LAUNCH(launch_enet_eval_pairs(a, (hipStream_t)stream), "enet_eval_pairs");
}

// S, f and border limits shared by the entry points; `who` prefixes the message
static int srcnn_pairs_limits(const char* who, int S, int f) {
    if (S < kSrcnnMinS || S > kSrcnnMaxS) return fail(SRX_ERR_BAD_ARG, "%s: S %d outside %d..%d", who, S, kSrcnnMinS, kSrcnnMaxS);
    if (f < 2) return fail(SRX_ERR_BAD_ARG, "%s: f %d below 2", who, f);
    if (S / f < 1) return fail(SRX_ERR_BAD_ARG, "%s: f %d gives S / f = %d / %d below 1", who, f, S, f);
    return SRX_OK;
}
static int srcnn_pairs_border_limits(const char* who, int S, int border) {
    if (!srcnn_pairs_border_ok(S, border)) return fail(SRX_ERR_BAD_ARG, "%s: border %d is negative or leaves nothing of S %d", who, border, S);
    return SRX_OK;
}

int srx_srcnn_pairs_band(int S, int f) {
    if (srcnn_pairs_limits("srcnn_pairs_band", S, f)) return -1;
    return srcnn_pairs_band(S, f);
}

int srx_srcnn_pairs_lds_bytes(int S, int f) {
    if (srcnn_pairs_limits("srcnn_pairs_lds_bytes", S, f)) return -1;
    return srcnn_pairs_lds(S, f).bytes;
}

int srx_srcnn_patch_table_check(const srx_patch_src* table_host, int B, int S, int f, int border, size_t arena_bytes) {
    if (!table_host) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_table_check: null table");
    if (B < 1 || B > kSrcnnMaxB) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_table_check: B %d outside 1..%d", B, kSrcnnMaxB);
    if (int rc = srcnn_pairs_limits("srcnn_patch_table_check", S, f)) return rc;
    if (int rc = srcnn_pairs_border_limits("srcnn_patch_table_check", S, border)) return rc;
    for (int e = 0; e < B; ++e) {
        const srx_patch_src& t = table_host[e];
        if (int rc = patch_entry_geometry("srcnn_patch_table_check", e, t, S, "crop", arena_bytes)) return rc;
        if (t.flip != 0 && t.flip != 1) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_table_check: entry %d: flip %d is not 0 or 1", e, t.flip);
        if (!(t.scaling_factor == (float)f))
            return fail(SRX_ERR_BAD_ARG, "srcnn_patch_table_check: entry %d: scaling factor %g is not the table's f %d", e,
                        (double)t.scaling_factor, f);
    }
    return SRX_OK;
}

int srx_srcnn_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S, int f, int border, float* sd, float* hd,
                          srx_stream_t stream) {
    if (!arena || !table_dev || !sd || !hd) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_pairs: null pointer");
    if (B < 1 || B > kSrcnnMaxB) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_pairs: B %d outside 1..%d", B, kSrcnnMaxB);
    if (int rc = srcnn_pairs_limits("srcnn_patch_pairs", S, f)) return rc;
    if (int rc = srcnn_pairs_border_limits("srcnn_patch_pairs", S, border)) return rc;
    if (sd == hd) return fail(SRX_ERR_BAD_ARG, "srcnn_patch_pairs: sd and hd must be distinct");
    if (!launch_srcnn_patch_pairs) return fail(SRX_ERR_UNSUPPORTED, "srcnn_patch_pairs: this build has no patch-pair kernel");
    const int s = S / f;
    // the scales as srx_resize_bicubic_tf forms them: (float)IN / (float)OUT
    const SrcnnPairsArgs a = {arena, table_dev, sd, hd, S, f, border, (float)S / (float)s, (float)s / (float)S};
    SRX_CHECK_LAUNCH(launch_srcnn_patch_pairs(a, B, (hipStream_t)stream), "srcnn_patch_pairs");
}

// ---- SRCNN's whole-image pairs (srcnn/srcnn.py:89-93,132-139; srcnn_eval.hip) ----

// f and border limits shared by the check, the footprint and the entry point; `who` prefixes the message
static int srcnn_eval_limits(const char* who, int f, int border) {
    if (!srcnn_eval_factor_ok(f)) return fail(SRX_ERR_BAD_ARG, "%s: f %d outside %d..%d", who, f, kSrcnnEvalMinF, kSrcnnEvalMaxF);
    if (border < 0) return fail(SRX_ERR_BAD_ARG, "%s: border %d is negative", who, border);
    return SRX_OK;
}

// One axis of a record for srx_srcnn_eval_table_check: the largest n_src, n_lo and n_out over its tiles (patch_pairs.h:
// srcnn_eval_axis), and that every tile's ranges are ordered and inside the image -- which the monotone floor and the clamps
// guarantee, and which is what the kernel's reads rely on.  O(side / T).
struct SrcnnEvalAxisMax {
    int n_src, n_lo, n_out;
    bool sane;
};
static SrcnnEvalAxisMax srcnn_eval_axis_max(int side, int f) {
    SrcnnEvalAxisMax m = {0, 0, 0, true};
    const int L = side / f;
    for (int k = 0; k < eval_tiles_along(side, SRX_SRCNN_EVAL_TILE); ++k) {
        const SrcnnEvalAxis a = srcnn_eval_axis(side, f, k);
        m.n_src = a.n_src > m.n_src ? a.n_src : m.n_src;
        m.n_lo = a.n_lo > m.n_lo ? a.n_lo : m.n_lo;
        m.n_out = a.n_out > m.n_out ? a.n_out : m.n_out;
        m.sane = m.sane && 0 <= a.lo_first && a.lo_first <= a.lo_last && a.lo_last < L && 0 <= a.src_first && a.src_first <= a.src_last &&
                 a.src_last < side;
    }
    m.sane = m.sane && m.n_src <= kSrcnnEvalMaxReach && m.n_lo <= kSrcnnEvalMaxReach && m.n_out <= kSrcnnEvalMaxReach;
    return m;
}

// What srx_srcnn_eval_table_check holds a table to
struct SrcnnEvalBounds {
    int f, border;
    size_t arena_bytes, out_floats, crop_floats;
};

// The walk srx_srcnn_eval_table_check and srx_srcnn_eval_tiles share, as vdsr_eval_walk: the table's arguments, every
// entry's sides and the tile count, which never passes kEvalMaxTiles.  With `bounds` (the check) the factor and the border
// are held to their limits, every entry to them, the arena, the running sums and the LDS layout, and the totals to
// out_floats and crop_floats.
static_assert(sizeof(srx_srcnn_eval_image) == 40, "srx_srcnn_eval_image is 40 bytes (include/srx.h)");
static int srcnn_eval_walk(const char* who, const srx_srcnn_eval_image* table, int n, const SrcnnEvalBounds* bounds, uint64_t* tiles_out) {
    if (int rc = eval_table_args(who, table, n)) return rc;
    if (bounds)
        if (int rc = srcnn_eval_limits(who, bounds->f, bounds->border)) return rc;
    uint64_t tiles = 0;
    uint64_t start[2] = {0, 0}, end[2] = {0, 0};      // [0]: sd, [1]: bq and hd; start: where this entry must begin (padded)
    for (int e = 0; e < n; ++e) {
        const srx_srcnn_eval_image& t = table[e];
        if (t.width < 1 || t.height < 1 || t.width > kSrcnnEvalMaxSide || t.height > kSrcnnEvalMaxSide)
            return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels: each side must be in 1..%d", who, e, t.width, t.height,
                        kSrcnnEvalMaxSide);
        if (bounds) {
            const int f = bounds->f, border = bounds->border;
            if (!srcnn_eval_side_ok(t.width, f, border) || !srcnn_eval_side_ok(t.height, f, border))
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: image of %d x %d pixels has no low-resolution pixel at f %d or nothing inside a "
                            "border of %d", who, e, t.width, t.height, f, border);
            if (int rc = image_inside_arena(who, e, t.offset, t.width, t.height, bounds->arena_bytes)) return rc;
            if (t.reserved != 0) return fail(SRX_ERR_BAD_ARG, "%s: entry %d: reserved %u is not 0", who, e, t.reserved);
            if (int rc = eval_first_tile(who, e, t.first_tile, tiles)) return rc;
            const uint64_t offsets[2] = {t.out_offset, t.crop_offset};
            const uint64_t own[2] = {eval_image_floats(t.width, t.height), srcnn_eval_crop_floats(t.width, t.height, border)};
            const uint64_t totals[2] = {(uint64_t)bounds->out_floats, (uint64_t)bounds->crop_floats};
            static const char* const names[2] = {"out_offset", "crop_offset"};
            if (int rc = eval_padded_sums(who, e, 2, names, offsets, own, totals, start, end)) return rc;
            const SrcnnEvalAxisMax my = srcnn_eval_axis_max(t.height, f), mx = srcnn_eval_axis_max(t.width, f);
            const int need = my.sane && mx.sane ? srcnn_eval_lds(my.n_src, mx.n_src, my.n_lo, mx.n_lo, my.n_out, mx.n_out).bytes : 0;
            if (!my.sane || !mx.sane || need > kSrcnnEvalLdsBytes)
                return fail(SRX_ERR_BAD_ARG, "%s: entry %d: a tile's footprint (%d x %d source pixels, %d x %d low-resolution pixels: %d "
                            "bytes) is beyond the LDS layout of %d bytes", who, e, my.n_src, mx.n_src, my.n_lo, mx.n_lo, need, kSrcnnEvalLdsBytes);
        }
        if (int rc = eval_add_tiles(who, e, eval_image_tiles(t.width, t.height, SRX_SRCNN_EVAL_TILE), &tiles)) return rc;
    }
    if (bounds && (end[0] != (uint64_t)bounds->out_floats || end[1] != (uint64_t)bounds->crop_floats))
        return fail(SRX_ERR_BAD_ARG, "%s: the table's %d entries end at float %llu of sd and %llu of bq and hd, not at out_floats %zu and "
                    "crop_floats %zu", who, n, (unsigned long long)end[0], (unsigned long long)end[1], bounds->out_floats, bounds->crop_floats);
    *tiles_out = tiles;
    return SRX_OK;
}

int srx_srcnn_eval_table_check(const srx_srcnn_eval_image* table_host, int n, int f, int border, size_t arena_bytes, size_t out_floats,
                               size_t crop_floats) {
    const SrcnnEvalBounds bounds = {f, border, arena_bytes, out_floats, crop_floats};
    uint64_t tiles = 0;
    return srcnn_eval_walk("srcnn_eval_table_check", table_host, n, &bounds, &tiles);
}

size_t srx_srcnn_eval_tiles(const srx_srcnn_eval_image* table_host, int n) {
    uint64_t tiles = 0;
    if (srcnn_eval_walk("srcnn_eval_tiles", table_host, n, nullptr, &tiles)) return 0;
    return (size_t)tiles;
}

int srx_srcnn_eval_footprint(int side, int f, int tile, int out[4]) {
    if (!out) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_footprint: null out");
    if (int rc = srcnn_eval_limits("srcnn_eval_footprint", f, 0)) return rc;
    if (side < 1 || side > kSrcnnEvalMaxSide) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_footprint: side %d outside 1..%d", side, kSrcnnEvalMaxSide);
    if (side / f < 1) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_footprint: a side of %d pixels has no low-resolution pixel at f %d", side, f);
    if (tile < 0 || tile >= eval_tiles_along(side, SRX_SRCNN_EVAL_TILE))
        return fail(SRX_ERR_BAD_ARG, "srcnn_eval_footprint: tile %d outside 0..%d", tile, eval_tiles_along(side, SRX_SRCNN_EVAL_TILE) - 1);
    const SrcnnEvalAxis a = srcnn_eval_axis(side, f, tile);
    out[0] = a.lo_first; out[1] = a.lo_last; out[2] = a.src_first; out[3] = a.src_last;
    return SRX_OK;
}

int srx_srcnn_eval_pairs(const uint8_t* arena, const srx_srcnn_eval_image* table_dev, int n, int f, int border, float* sd, float* bq,
                         float* hd, srx_stream_t stream) {
    if (!arena || !table_dev || !sd || !bq || !hd) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_pairs: null pointer");
    if (n < 1) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_pairs: n %d below 1", n);
    if (int rc = srcnn_eval_limits("srcnn_eval_pairs", f, border)) return rc;
    if (sd == bq || sd == hd || bq == hd) return fail(SRX_ERR_BAD_ARG, "srcnn_eval_pairs: sd, bq and hd must be distinct");
    if (!launch_srcnn_eval_pairs) return fail(SRX_ERR_UNSUPPORTED, "srcnn_eval_pairs: this build has no eval-pair kernel");
    const SrcnnEvalArgs a = {arena, table_dev, sd, bq, hd, n, f, border};
    SRX_CHECK_LAUNCH(launch_srcnn_eval_pairs(a, (hipStream_t)stream), "srcnn_eval_pairs");
}

}  // extern "C"
