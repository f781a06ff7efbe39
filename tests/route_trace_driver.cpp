// Test driver (CPU only) for tests/test_routes_host.py: linked with a plain --cuda-host-only build of srx_api.hip and
// the stubs of host_stubs.h, it records WHICH launchers every convolution entry point offers a shape to, in which
// order and with which arguments.  Nothing is allocated and no HIP runtime is started: tensors are fake addresses,
// printed as offsets, so any dimension costs nothing.
//
// Every case runs under several acceptance masks: every launcher refuses (the whole ladder, in order), every launcher
// accepts (the first offer), every launcher accepts and reports a launch error, only the reductions report one, and
// each launcher that the ladder offered accepts alone.  A case prints the host-only queries for its descriptor, then
// per mask the trace, the return code, srx_last_error() and n_partials.
//
//   route_trace_driver                 the full output of every case, in this process's environment
//   route_trace_driver --case NAME     ... of one case
//   route_trace_driver --fwd N H W CIN COUT K PAD   ... of a forward layer that is no case (PAD: 0 SAME, 1 VALID): what a GPU test's
//                                      shape is planned as; not part of the golden file
//   route_trace_driver --hashes        one line per case: its name and the 64-bit FNV-1a hash of its output
//   route_trace_driver --coverage      per launcher: times offered / accepted; then every distinct error text seen
//   route_trace_driver --all           the full output under every configuration (CU counts, one environment knob each)
//   route_trace_driver --record        the golden file tests/golden/conv_routes.txt: per group of cases one hash over their
//                                      output under every configuration, and four digits per case
//   route_trace_driver --time          nanoseconds per stubbed call on the VDSR body shape (host overhead)
// The knobs are read once per process, so --all and --record start this program again for every configuration.
// ROUTE_TRACE_CUS: the CU count the stubbed runtime reports (default 256).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#define SRX_STUB_WEAK_LAUNCHERS
#include "host_stubs.h"

using namespace srx;

namespace {

enum Mode { REFUSE_ALL, ACCEPT_ALL, ERR_LAUNCH, ERR_REDUCE, ONE_HOT, QUIET };
Mode g_mode = REFUSE_ALL;
int g_hot = -1;
std::string g_text;                      // the running case's output
long g_lines = 0, g_folded = 0;          // trace lines of the running mask; those past the cap are hashed, not kept
uint64_t g_fold_hash = 0;
constexpr long kLineCap = 48;
bool g_offered_now[srx_stub::kIds];
long g_offered[srx_stub::kIds], g_accepted[srx_stub::kIds];
std::set<std::string> g_errors;

uint64_t fnv(const char* s, size_t n, uint64_t h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; ++i) { h ^= (unsigned char)s[i]; h *= 1099511628211ull; }
    return h;
}

void out(const char* fmt, ...) {
    char buf[8192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_text += buf;
}

// fake tensors: region i of 2^36 bytes above 2^40; printed as region:offset
constexpr uintptr_t kBase = (uintptr_t)1 << 40, kSpan = (uintptr_t)1 << 36;
float* T(int i, size_t off_floats = 0) { return (float*)(kBase + (uintptr_t)i * kSpan) + off_floats; }
std::string P(const void* p) {
    if (!p) return "-";
    char b[48];
    const uintptr_t v = (uintptr_t)p - kBase;
    snprintf(b, sizeof(b), "T%d:%llx", (int)(v / kSpan), (unsigned long long)(v % kSpan));
    return b;
}
enum { X = 0, WT, BIAS, SKIP, MASK, Y, WS, DW, DB, DECAY, LAYERS };

std::string line_of(const srx_stub::Call& c) {
    char b[8192];
    int n = snprintf(b, sizeof(b), "%s", srx_stub::name(c.id));
    auto add = [&](const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        if (n < (int)sizeof(b)) n += vsnprintf(b + n, sizeof(b) - n, fmt, ap);
        va_end(ap);
    };
    auto opt = [&](const char* what, long v) { if (v >= 0) add(" %s=%ld", what, v); };
    if (c.key) add(" key=%d,%d,%d,%d,%d", c.key->kh, c.key->kw, c.key->cinp, c.key->nch, (int)c.key->wt);
    opt("grid", c.grid); opt("lds", c.lds); opt("min_pixels", c.min_pixels); opt("max_partials", c.max_partials);
    opt("wt", c.wt); opt("aux", c.aux); opt("fixed", c.fixed); opt("wpl", c.wpl); opt("layers", c.layers); opt("G", c.G);
    opt("pairs", c.pairs); opt("strips", c.strips); opt("stride", c.stride); opt("wn", c.wn); opt("cout", c.cout); opt("cob", c.cob);
    if (c.dims[0] >= 0) add(" NHW=%d,%d,%d relu=%d", c.dims[0], c.dims[1], c.dims[2], c.dims[3]);
    if (c.id == srx_stub::k_reduce_partials || c.id == srx_stub::k_wgrad_batch_reduce) add(" wd=%a", (double)c.wd);
    for (int i = 0; i < c.n_ptr; ++i) add(" p%d=%s", i, P(c.ptr[i]).c_str());
    if (c.conv) {
        const ConvArgs& a = *c.conv;
        add(" | x=%s w=%s bias=%s skip=%s mask=%s y=%s N=%d H=%d W=%d OH=%d OW=%d Cin=%d Cout=%d pad=%d,%d TH=%d TW=%d NTX=%d RS=%d units=%d"
            " act=%d post_relu=%d mask_act=%d inv_rs=%a stagger=%d dbg=%d trace=%s buf_floats=%d stride=%d d2s=%d,%d",
            P(a.x).c_str(), P(a.w).c_str(), P(a.bias).c_str(), P(a.skip).c_str(), P(a.mask).c_str(), P(a.y).c_str(), a.N, a.H, a.W, a.OH,
            a.OW, a.Cin, a.Cout, a.pad_t, a.pad_l, a.TH, a.TW, a.NTX, a.RS, a.units_total, a.act, a.post_relu, a.mask_act, (double)a.inv_rs,
            a.stagger, a.dbg, P(a.trace).c_str(), a.buf_floats, a.stride, a.d2s_r, a.d2s_rc);
    }
    if (c.wgrad) {
        const WgradArgs& a = *c.wgrad;
        add(" | x=%s dpre=%s part=%s part_stride=%d N=%d H=%d W=%d OH=%d OW=%d Cin=%d Cout=%d pad=%d,%d TH=%d TW=%d NTX=%d RS=%d units=%d"
            " inv_rs=%a stagger=%d zero_slot=%d stride=%d trace=%s",
            P(a.x).c_str(), P(a.dpre).c_str(), P(a.part).c_str(), a.part_stride, a.N, a.H, a.W, a.OH, a.OW, a.Cin, a.Cout, a.pad_t, a.pad_l,
            a.TH, a.TW, a.NTX, a.RS, a.units_total, (double)a.inv_rs, a.stagger, a.zero_slot, a.stride, P(a.trace).c_str());
    }
    if (c.pairs_args) add(" | x_pair=%ld d_pair=%ld part_pair=%ld cob=%d", c.pairs_args->x_pair_stride, c.pairs_args->d_pair_stride,
                          c.pairs_args->part_pair_stride, c.pairs_args->cob);
    if (c.bf3) add(" | bf3 TH=%d TW=%d ntx=%d nty=%d tiles=%d grid=%d lds=%zu", c.bf3->TH, c.bf3->TW, c.bf3->ntx, c.bf3->nty, c.bf3->tiles,
                   c.bf3->grid, c.bf3->lds);
    if (c.chain) {
        add(" | L=%d", c.chain->L);
        for (int l = 0; l < kChainMax; ++l)
            if (c.chain->x[l] || c.chain->w[l] || c.chain->bias[l] || c.chain->aux[l] || c.chain->y[l])
                add(" [%d %s %s %s %s %s]", l, P(c.chain->x[l]).c_str(), P(c.chain->w[l]).c_str(), P(c.chain->bias[l]).c_str(),
                    P(c.chain->aux[l]).c_str(), P(c.chain->y[l]).c_str());
    }
    if (c.batch)
        for (int l = 0; l < kChainMax; ++l)
            if (c.batch->x[l] || c.batch->dpre[l]) add(" [%d %s %s]", l, P(c.batch->x[l]).c_str(), P(c.batch->dpre[l]).c_str());
    if (c.batch_out)
        for (int l = 0; l < kChainMax; ++l)
            if (c.batch_out->dw[l] || c.batch_out->dbias[l] || c.batch_out->w[l])
                add(" [%d %s %s %s]", l, P(c.batch_out->dw[l]).c_str(), P(c.batch_out->dbias[l]).c_str(), P(c.batch_out->w[l]).c_str());
    return b;
}

// (past the cap -- the per-pair fallback of 65,792 block pairs -- a call adds its launcher and answer to a hash, no line)
void trace(const srx_stub::Call& c, const char* answer) {
    if (g_lines++ < kLineCap) { g_text += "  " + line_of(c) + " -> " + answer + "\n"; return; }
    const char l[2] = {(char)c.id, answer[0]};
    g_folded++;
    g_fold_hash = fnv(l, 2, g_fold_hash ? g_fold_hash : 1469598103934665603ull);
}

bool is_reduce(int id) { return id == srx_stub::k_reduce_partials || id == srx_stub::k_reduce_partials_pairs || id == srx_stub::k_wgrad_batch_reduce; }

}  // namespace

namespace srx_stub {
bool offer(const Call& c, hipError_t* err) {
    // (--time: the VDSR body layer's own launchers take it, every offer before them is refused as on the device)
    if (g_mode == QUIET) { *err = hipSuccess; return c.id == k_pipe_k3c64 || c.id == k_wgrad_rows_full; }
    const bool take = g_mode == ACCEPT_ALL || g_mode == ERR_LAUNCH || g_mode == ERR_REDUCE || (g_mode == ONE_HOT && g_hot == c.id);
    g_offered_now[c.id] = true;
    g_offered[c.id]++;
    if (take) {
        g_accepted[c.id]++;
        *err = g_mode == ERR_LAUNCH ? hipErrorLaunchFailure : hipSuccess;
        if (c.n_partials) *c.n_partials = c.max_partials > 1 ? (int)c.max_partials / 2 : 1;
    }
    trace(c, take ? (g_mode == ERR_LAUNCH ? "error" : "taken") : "refused");
    return take;
}
hipError_t call(const Call& c) {
    if (g_mode == QUIET || c.id == k_elementwise) return hipSuccess;
    const bool bad = is_reduce(c.id) ? g_mode == ERR_REDUCE : g_mode == ERR_LAUNCH;
    g_offered[c.id]++;
    if (!bad) g_accepted[c.id]++;
    trace(c, bad ? "error" : "ok");
    return bad ? hipErrorLaunchFailure : hipSuccess;
}
int cu_count() { const char* e = getenv("ROUTE_TRACE_CUS"); return e ? atoi(e) : 256; }
}  // namespace srx_stub

namespace {

// ---- cases ----------------------------------------------------------------------------------------------------------
struct Sw { int conv_path = -2, wgrad_path = -2, chain = -2, chain_fixed = -2, wgrad_batch = -2; };   // -2: leave alone
struct Case {
    std::string name;
    Sw sw;
    bool has_desc;
    srx_conv_desc d;
    std::function<int(int*)> run;     // one call of an entry point; *n_partials where there is one (else left at -1)
};
std::vector<Case> g_cases;

srx_conv_desc D(int N, int H, int W, int Cin, int Cout, int K, int stride = 1, int pad = SRX_PAD_SAME, int act = SRX_ACT_NONE) {
    srx_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = N; d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout; d.KH = K; d.KW = K; d.stride = stride; d.pad_mode = pad; d.act = act;
    return d;
}
std::string dname(const srx_conv_desc& d) {
    char b[160];
    int n = snprintf(b, sizeof(b), "%dx%dx%dx%d->%d_k%d", d.N, d.H, d.W, d.Cin, d.Cout, d.KH);
    auto opt = [&](const char* what, int v, int dflt) { if (v != dflt) n += snprintf(b + n, sizeof(b) - n, "_%s%d", what, v); };
    opt("kw", d.KW, d.KH); opt("s", d.stride, 1); opt("valid", d.pad_mode, 0); opt("a", d.act, 0); opt("pa", d.post_add_relu, 0);
    opt("p", d.precision, 0); opt("r", d.subpixel_r, 0);
    return b;
}
constexpr size_t kBigWs = (size_t)1 << 35;

void add_case(const std::string& name, const srx_conv_desc* d, std::function<int(int*)> run, Sw sw = Sw()) {
    Case c;
    char b[96] = "";
    if (sw.conv_path != -2 || sw.wgrad_path != -2 || sw.chain != -2 || sw.chain_fixed != -2 || sw.wgrad_batch != -2)
        snprintf(b, sizeof(b), "/sw%d,%d,%d,%d,%d", sw.conv_path, sw.wgrad_path, sw.chain, sw.chain_fixed, sw.wgrad_batch);
    c.name = name + b; c.sw = sw; c.has_desc = d != nullptr;
    if (d) c.d = *d; else memset(&c.d, 0, sizeof(c.d));
    c.run = run;
    g_cases.push_back(c);
}
void fwd(const std::string& tag, srx_conv_desc d, bool skip = false, Sw sw = Sw(), bool inplace = false) {
    add_case(tag + "/fwd" + (skip ? "+skip" : "") + (inplace ? "+inplace" : "") + "/" + dname(d), &d, [=](int*) {
        return srx_conv2d_fwd(&d, T(X), T(WT), T(BIAS), skip ? (inplace ? T(Y) : T(SKIP)) : nullptr, T(Y), nullptr, 0, nullptr);
    }, sw);
}
// mask: 0 none, 1 x_in, 2 x_in == dx_out (in place); acc: srx_conv2d_bwd_data_acc
void dgrad(const std::string& tag, srx_conv_desc d, int in_act = SRX_ACT_NONE, int mask = 0, bool acc = false, Sw sw = Sw()) {
    char b[64];
    snprintf(b, sizeof(b), "/dgrad_ia%d_m%d%s/", in_act, mask, acc ? "_acc" : "");
    add_case(tag + b + dname(d), &d, [=](int*) {
        if (acc) return srx_conv2d_bwd_data_acc(&d, T(X), T(WT), T(SKIP), T(Y), nullptr, 0, nullptr);
        return srx_conv2d_bwd_data(&d, T(X), T(WT), mask ? (mask == 2 ? T(Y) : T(MASK)) : nullptr, in_act, T(Y), nullptr, 0, nullptr);
    }, sw);
}
void wgrad(const std::string& tag, srx_conv_desc d, Sw sw = Sw()) {
    add_case(tag + "/wgrad/" + dname(d), &d, [=](int* n) {
        int rc = srx_conv2d_bwd_filter_partials(&d, T(X), T(Y), T(WS), kBigWs, n, nullptr);
        if (rc) return rc;
        return srx_conv2d_bwd_filter_reduce(&d, T(WS), *n, T(DW), T(DB), T(DECAY), 0.5f, nullptr);
    }, sw);
}
void all3(const std::string& tag, srx_conv_desc d, int in_act = SRX_ACT_NONE, Sw sw = Sw()) {
    fwd(tag, d, false, sw);
    srx_conv_desc b = d;
    b.act = 0;
    if (d.stride == 1) dgrad(tag, b, in_act, in_act ? 1 : 0, false, sw);
    wgrad(tag, b, sw);
}
// what: 0 plain; 1 null arrays; 2 null tensor in layer 1; 3 unaligned; 4 y == x; 5 forward with an aux operand; 6 mask without ReLU
void chain(const std::string& tag, srx_conv_desc d, int op, int in_act, int layers, int what = 0, Sw sw = Sw()) {
    char b[64];
    snprintf(b, sizeof(b), "/chain_op%d_ia%d_L%d_w%d/", op, in_act, layers, what);
    add_case(tag + b + dname(d), &d, [=](int*) {
        const float *x[40], *w[40], *bias[40], *aux[40];
        float* y[40];
        for (int l = 0; l < 40; ++l) {
            x[l] = T(LAYERS + 0, (size_t)l << 24); w[l] = T(LAYERS + 1, (size_t)l << 24); bias[l] = T(LAYERS + 2, (size_t)l << 8);
            aux[l] = T(LAYERS + 3, (size_t)l << 24); y[l] = T(LAYERS + 4, (size_t)l << 24);
        }
        if (what == 2) w[1] = nullptr;
        if (what == 3) x[0] = (const float*)((const char*)x[0] + 4);
        if (what == 4) y[0] = (float*)x[0];
        const bool want_aux = (op == SRX_OP_BWD_DATA && in_act == SRX_ACT_RELU) || what == 5;
        return srx_conv_chain(&d, op, in_act, layers, what == 1 ? nullptr : x, w, bias, (want_aux && what != 6) || (what == 6 && !want_aux) ? aux : nullptr, y, nullptr);
    }, sw);
}
// what: 0 plain; 1 null arrays; 2 null tensor in layer 1; 3 unaligned; 4 small workspace; 5 unaligned workspace
void batch(const std::string& tag, srx_conv_desc d, int layers, int what = 0, Sw sw = Sw()) {
    char b[64];
    snprintf(b, sizeof(b), "/batch_L%d_w%d/", layers, what);
    add_case(tag + b + dname(d), &d, [=](int*) {
        const float *x[40], *dp[40], *wd[40];
        float *dw[40], *db[40];
        for (int l = 0; l < 40; ++l) {
            x[l] = T(LAYERS + 0, (size_t)l << 24); dp[l] = T(LAYERS + 1, (size_t)l << 24); wd[l] = T(LAYERS + 2, (size_t)l << 20);
            dw[l] = T(LAYERS + 3, (size_t)l << 20); db[l] = (l & 1) ? nullptr : T(LAYERS + 4, (size_t)l << 8);
        }
        if (what == 2) dp[1] = nullptr;
        if (what == 3) dw[0] = (float*)((char*)dw[0] + 4);
        return srx_conv2d_bwd_filter_batch(&d, layers, what == 1 ? nullptr : x, dp, dw, db, wd, 0.25f, what == 5 ? (void*)((char*)T(WS) + 4) : T(WS),
                                           what == 4 ? 64 : kBigWs, nullptr);
    }, sw);
}
// what: 0 plain; 1 null tensor; 2 unaligned; 3 small workspace
void blocked(const std::string& tag, int N, int H, int W, int sb, int pb, int precision, int what = 0, Sw sw = Sw()) {
    char b[128];
    snprintf(b, sizeof(b), "/blocked_%dx%dx%d_%dx%d_p%d_w%d", N, H, W, sb, pb, precision, what);
    add_case(tag + b, nullptr, [=](int*) {
        out("  blocked_ws=%zu blocked_ex_ws=%zu\n", srx_conv3x3_blocked_bwd_filter_workspace_bytes(N, H, W, sb, pb),
            srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(N, H, W, sb, pb, precision));
        const float* x = what == 1 ? nullptr : (what == 2 ? (const float*)((const char*)T(X) + 4) : T(X));
        const size_t ws = what == 3 ? 64 : kBigWs;
        if (precision < 0) return srx_conv3x3_blocked_bwd_filter(x, T(Y), T(DW), T(DB), N, H, W, sb, pb, T(WS), ws, nullptr);
        return srx_conv3x3_blocked_bwd_filter_ex(x, T(Y), T(DW), T(DB), N, H, W, sb, pb, precision, T(WS), ws, nullptr);
    }, sw);
}

void build_cases() {
    const int R = SRX_ACT_RELU, TANH = SRX_ACT_TANH, LRELU = SRX_ACT_LRELU, SIG = SRX_ACT_SIGMOID, VALID = SRX_PAD_VALID, SAME = SRX_PAD_SAME;
    // ---- every model's layers, at patch size and at whole-image size
    for (int N : {1, 16, 64, 256, 300, 512}) {
        all3("vdsr", D(N, 41, 41, 3, 64, 3, 1, SAME, R));
        all3("vdsr", D(N, 41, 41, 64, 64, 3, 1, SAME, R), R);
        all3("vdsr", D(N, 41, 41, 64, 3, 3), R);
    }
    all3("vdsr", D(1, 720, 1280, 3, 64, 3, 1, SAME, R));
    all3("vdsr", D(1, 720, 1280, 64, 64, 3, 1, SAME, R), R);
    all3("vdsr", D(1, 720, 1280, 64, 3, 3), R);
    const int espcn[][3] = {{64, 17, 17}, {1, 256, 256}, {1, 720, 1280}};
    for (auto& s : espcn) {
        all3("espcn", D(s[0], s[1], s[2], 3, 64, 5, 1, SAME, TANH));
        all3("espcn", D(s[0], s[1], s[2], 64, 32, 3, 1, SAME, TANH), TANH);
        srx_conv_desc f3 = D(s[0], s[1], s[2], 32, 27, 3);
        f3.subpixel_r = 3;
        fwd("espcn", f3);
        f3.subpixel_r = 0;
        all3("espcn", f3, TANH);
    }
    const int srcnn[][3] = {{128, 33, 33}, {1, 720, 1280}};
    for (auto& s : srcnn) {
        all3("srcnn", D(s[0], s[1], s[2], 3, 64, 9, 1, VALID, R));
        all3("srcnn", D(s[0], s[1] - 8, s[2] - 8, 64, 32, 1, 1, VALID, R), R);
        all3("srcnn", D(s[0], s[1] - 8, s[2] - 8, 32, 3, 5, 1, VALID), R);
        all3("srcnn", D(s[0], s[1], s[2], 3, 64, 9, 1, SAME, R));
        all3("srcnn", D(s[0], s[1], s[2], 32, 3, 5, 1, SAME), R);
    }
    const int enet[][3] = {{64, 32, 32}, {16, 128, 128}, {16, 33, 33}, {4, 127, 129}};
    for (auto& s : enet) {
        all3("enet", D(s[0], s[1], s[2], 32, 32, 3, 2, SAME, LRELU));
        all3("enet", D(s[0], s[1], s[2], 64, 64, 3, 2, SAME, LRELU));
        all3("enet", D(s[0], s[1], s[2], 64, 64, 2, 1, SAME, R), R);
        all3("enet", D(s[0], s[1], s[2], 64, 64, 4, 1, SAME, R), R);
        all3("enet", D(s[0], s[1], s[2], 3, 32, 4, 2, SAME, R));
        if (s[1] & 1) continue;      // (odd sizes: the layers above, whose padding depends on them)
        all3("enet", D(s[0], s[1], s[2], 3, 64, 3, 1, SAME, R));
        all3("enet", D(s[0], s[1], s[2], 64, 64, 3, 1, SAME, R), R);
        srx_conv_desc res = D(s[0], s[1], s[2], 64, 64, 3);
        fwd("enet", res, true);
        res.post_add_relu = R;
        fwd("enet", res, true);
        all3("enet", D(s[0], s[1], s[2], 64, 64, 1, 1, SAME, R), R);
        all3("enet", D(s[0], s[1], s[2], 64, 3, 3), R);
        all3("enet", D(s[0], s[1], s[2], 3, 32, 3, 1, SAME, LRELU), LRELU);
        all3("enet", D(s[0], s[1], s[2], 32, 64, 3, 1, SAME, LRELU), LRELU);
        all3("enet", D(s[0], s[1], s[2], 64, 1, 3, 1, SAME, SIG), LRELU);
    }
    // ---- widths around every threshold of a predicate; one to three rows
    for (int W : {3, 4, 7, 8, 15, 16, 31, 32, 33, 41, 42}) {
        all3("width", D(4, 17, W, 64, 64, 3, 1, SAME, R), R);
        all3("width", D(4, 17, W, 32, 32, 3, 1, SAME, R), R);
        for (int H : {1, 2, 3})
            if (W == 4 || W == 16 || W == 41) all3("width", D(4, H, W, 64, 64, 3, 1, SAME, R), R);
    }
    // ---- column strips whose last strip is 0, 1, 3, 4 and 5 columns wide (64 channels: from 60 columns; 32: from 114)
    for (int r : {0, 1, 3, 4, 5}) {
        all3("strip", D(2, 40, 64 + r, 64, 64, 3, 1, SAME, R), R);
        all3("strip", D(2, 40, 128 + r, 32, 32, 3, 1, SAME, R), R);
        all3("strip", D(2, 40, 128 + r, 64, 32, 3, 1, SAME, TANH), R);
    }
    all3("strip", D(2, 2, 97, 64, 64, 3, 1, SAME, R), R);
    all3("strip", D(2, 40, 65, 64, 64, 5, 1, SAME, R), R);
    all3("strip", D(2, 40, 59, 64, 64, 3, 1, SAME, R), R);
    all3("strip", D(2, 40, 60, 64, 64, 3, 1, SAME, R), R);
    all3("strip", D(2, 40, 113, 32, 32, 3, 1, SAME, R), R);
    all3("strip", D(2, 40, 114, 32, 32, 3, 1, SAME, R), R);
    // ---- channel counts that are no multiple of 4, and above 64
    const int chans[][2] = {{3, 64}, {64, 3}, {1, 64}, {5, 7}, {16, 16}, {17, 33}, {32, 27}, {48, 64}, {64, 48}, {33, 64}, {65, 64}, {64, 65}, {64, 62}, {4, 4}, {62, 64}};
    for (auto& c : chans) {
        all3("chan", D(8, 24, 24, c[0], c[1], 3, 1, SAME, R), R);
        if (c[0] + c[1] < 64 || c[1] == 3) all3("chan", D(2, 200, 200, c[0], c[1], 3, 1, SAME, R), R);
    }
    // ---- every activation, skip, post-add and mask form the epilogue predicates mention
    for (int W : {41, 128})
        for (int act = 0; act <= 4; ++act) {
            for (int pa : {0, (int)SRX_ACT_RELU, (int)SRX_ACT_LRELU})
                for (int skip = 0; skip < 2; ++skip) {
                    srx_conv_desc d = D(16, 41, W, 64, 64, 3, 1, SAME, act);
                    d.post_add_relu = pa;
                    fwd("epi", d, skip != 0);
                }
            for (int mask = 0; mask < 3; ++mask) dgrad("epi", D(16, 41, W, 64, 64, 3), act, mask);
        }
    for (int W : {41, 128}) {
        dgrad("epi", D(16, 41, W, 64, 64, 3), 0, 0, true);
        fwd("epi", D(16, 41, W, 64, 64, 3), true, Sw(), true);
        srx_conv_desc d = D(16, 41, W, 64, 32, 3, 1, SAME, TANH);
        fwd("epi", d, true);
        d.post_add_relu = R;
        fwd("epi", d, false);
    }
    // ---- the data gradient of a VALID layer; the 32-wide 64-channel tile that fills the LDS budget
    all3("valid", D(16, 41, 41, 64, 64, 3, 1, VALID, R), R);
    all3("valid", D(16, 41, 128, 64, 64, 3, 1, VALID, R), R);
    all3("valid", D(16, 41, 41, 32, 32, 5, 1, VALID, R), R);
    all3("budget", D(64, 32, 32, 64, 64, 3, 1, SAME, R), R);
    all3("budget", D(1024, 32, 32, 64, 64, 3, 1, SAME, R), R);
    all3("budget", D(64, 32, 32, 32, 64, 3, 1, SAME, R), R);
    // ---- just below and above each 2^30 / 2^31 bound
    for (int W : {4095, 4096, 4097}) all3("bound", D(1, 2048, W, 64, 64, 3, 1, SAME, R), R);         // H W C 4 against 2^31 - 64
    for (int W : {1048573, 1048574, 1048575}) all3("bound", D(1, 8, W, 64, 64, 3, 1, SAME, R), R);   // ... and 2^31 - 4096
    for (int W : {2047, 2048, 2049}) all3("bound", D(1, 2048, W, 64, 64, 3, 1, SAME, R), R);         // OH OW Cout 4 against 2^30
    for (int W : {4854, 4855}) { srx_conv_desc d = D(1, 4096, W, 32, 27, 3); d.subpixel_r = 3; fwd("bound", d); }   // the sub-pixel store's 2^31
    for (int H : {5792, 5793}) all3("bound", D(1, H, H, 64, 64, 3, 1, SAME, R), R);                   // check_desc: one image, 2^31 elements
    for (int N : {65535, 65536}) all3("bound", D(N, 512, 4, 64, 64, 3, 1, SAME, R), R);               // check_desc: rows
    all3("bound", D(32768, 512, 16384, 4, 4, 3, 2, SAME, R));                                         // stride 2: tile rows
    all3("bound", D(2, 64, 64, 64, 64, 41, 1, SAME, R));                                              // filter too large for the tile
    all3("bound", D(2, 64, 64, 64, 64, 41, 2, SAME, R));
    // ---- precision 1
    for (int N : {1, 64, 300}) {
        srx_conv_desc d = D(N, 41, 41, 64, 64, 3, 1, SAME, R);
        d.precision = 1;
        all3("bf16x3", d, R);
    }
    {
        srx_conv_desc d = D(2, 128, 300, 64, 64, 3);
        d.precision = 1;
        all3("bf16x3", d);
        fwd("bf16x3", d, true);
        dgrad("bf16x3", d, 0, 0, true);
        dgrad("bf16x3", d, TANH, 1);
        srx_conv_desc e;
        e = d; e.KH = e.KW = 5; all3("bf16x3-no", e);
        e = d; e.Cin = 32; all3("bf16x3-no", e);
        e = d; e.stride = 2; all3("bf16x3-no", e);
        e = d; e.pad_mode = VALID; all3("bf16x3-no", e);
        e = d; e.post_add_relu = R; fwd("bf16x3-no", e);
        e = d; e.subpixel_r = 2; fwd("bf16x3-no", e);
        e = d; e.act = TANH; fwd("bf16x3-no", e);
        e = d; e.precision = 2; all3("bf16x3-no", e);
    }
    // ---- argument errors of the conv, data-gradient and filter-gradient entry points
    {
        const srx_conv_desc ok = D(4, 41, 41, 64, 64, 3, 1, SAME, R);
        srx_conv_desc e;
        e = ok; e.N = 0; all3("bad", e);
        e = ok; e.stride = 3; all3("bad", e);
        e = ok; e.stride = 2; e.subpixel_r = 2; fwd("bad", e);
        e = ok; e.pad_mode = 2; all3("bad", e);
        e = ok; e.act = 5; fwd("bad", e);
        e = ok; e.post_add_relu = 2; fwd("bad", e);
        e = ok; e.subpixel_r = 17; fwd("bad", e);
        e = ok; e.subpixel_r = 3; fwd("bad", e);
        e = ok; e.subpixel_r = 2; fwd("bad", e, true);
        e = D(4, 2, 2, 64, 64, 3, 1, VALID); all3("bad", e);
        dgrad("bad", ok, 5, 1);
        dgrad("bad", D(4, 41, 41, 64, 64, 3, 2), 0, 0);
        add_case("bad/null-desc", nullptr, [](int* n) {
            int rc = srx_conv2d_fwd(nullptr, T(X), T(WT), nullptr, nullptr, T(Y), nullptr, 0, nullptr);
            out("  fwd rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_data(nullptr, T(X), T(WT), nullptr, 0, T(Y), nullptr, 0, nullptr);
            out("  dgrad rc=%d err=\"%s\"\n", rc, srx_last_error());
            return srx_conv2d_bwd_filter_partials(nullptr, T(X), T(Y), T(WS), kBigWs, n, nullptr);
        });
        add_case("bad/null-tensors", &ok, [=](int* n) {
            int rc = srx_conv2d_fwd(&ok, nullptr, T(WT), nullptr, nullptr, T(Y), nullptr, 0, nullptr);
            out("  fwd rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_data(&ok, T(X), nullptr, nullptr, 0, T(Y), nullptr, 0, nullptr);
            out("  dgrad rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_data_acc(&ok, T(X), T(WT), nullptr, T(Y), nullptr, 0, nullptr);
            out("  dgrad_acc rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_filter(&ok, T(X), T(Y), nullptr, nullptr, nullptr, 0.f, T(WS), kBigWs, nullptr);
            out("  wgrad rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_filter_reduce(&ok, nullptr, 4, T(DW), nullptr, nullptr, 0.f, nullptr);
            out("  reduce rc=%d err=\"%s\"\n", rc, srx_last_error());
            for (int np : {0, 512, 513}) {
                rc = srx_conv2d_bwd_filter_reduce(&ok, T(WS), np, T(DW), nullptr, nullptr, 0.f, nullptr);
                out("  reduce n=%d rc=%d err=\"%s\"\n", np, rc, rc ? srx_last_error() : "");
            }
            return srx_conv2d_bwd_filter_partials(&ok, T(X), nullptr, T(WS), kBigWs, n, nullptr);
        });
        add_case("bad/alignment", &ok, [=](int* n) {
            float* odd = (float*)((char*)T(X) + 4);
            int rc = srx_conv2d_fwd(&ok, odd, T(WT), nullptr, nullptr, T(Y), nullptr, 0, nullptr);
            out("  fwd rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_fwd(&ok, T(X), T(WT), nullptr, odd, T(Y), nullptr, 0, nullptr);
            out("  fwd skip rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_data(&ok, T(X), T(WT), odd, 1, T(Y), nullptr, 0, nullptr);
            out("  dgrad rc=%d err=\"%s\"\n", rc, srx_last_error());
            rc = srx_conv2d_bwd_filter_partials(&ok, T(X), T(Y), odd, kBigWs, n, nullptr);
            out("  wgrad ws rc=%d err=\"%s\"\n", rc, srx_last_error());
            return srx_conv2d_bwd_filter_partials(&ok, T(X), odd, T(WS), kBigWs, n, nullptr);
        });
        for (int prec : {0, 1}) {
            srx_conv_desc w = ok;
            w.precision = prec;
            add_case("bad/workspace/" + dname(w), &w, [=](int* n) {
                int rc = srx_conv2d_bwd_filter_partials(&w, T(X), T(Y), nullptr, kBigWs, n, nullptr);
                out("  null ws rc=%d err=\"%s\"\n", rc, srx_last_error());
                if (prec) {
                    rc = srx_conv2d_bwd_filter_partials(&w, T(X), T(Y), (char*)T(WS) + 4, kBigWs, n, nullptr);
                    out("  odd ws rc=%d err=\"%s\"\n", rc, srx_last_error());
                }
                return srx_conv2d_bwd_filter_partials(&w, T(X), T(Y), T(WS), 1024, n, nullptr);
            });
        }
    }
    // ---- chains and batches: layer counts, N against the grid, every refusal
    {
        const srx_conv_desc body = D(256, 41, 41, 64, 64, 3, 1, SAME, R);
        for (int L : {0, 1, 2, 18, 32, 33})
            for (int N : {64, 256, 300, 512}) {
                srx_conv_desc d = body;
                d.N = N;
                if (N == 256 || L == 18) {
                    chain("chain", d, SRX_OP_FWD, 0, L);
                    chain("chain", d, SRX_OP_BWD_DATA, R, L);
                    chain("chain", d, SRX_OP_BWD_DATA, 0, L);
                }
                if (N == 64 || N == 300 || L == 18) batch("batch", d, L);
            }
        srx_conv_desc e;
        e = body; e.act = 0; chain("chain", e, SRX_OP_FWD, 0, 3);
        chain("chain-no", body, SRX_OP_BWD_FILTER, 0, 3);
        e = body; e.precision = 1; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.KH = e.KW = 5; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.Cin = 32; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.pad_mode = VALID; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.subpixel_r = 2; chain("chain-no", e, SRX_OP_FWD, 0, 3);
        e = body; e.post_add_relu = R; chain("chain-no", e, SRX_OP_FWD, 0, 3);
        e = body; e.act = TANH; chain("chain-no", e, SRX_OP_FWD, 0, 3); chain("chain-no", e, SRX_OP_BWD_DATA, 0, 3);
        chain("chain-no", body, SRX_OP_BWD_DATA, TANH, 3);
        e = body; e.W = 128; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.W = 15; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.N = 0; chain("chain-no", e, SRX_OP_FWD, 0, 3); batch("batch-no", e, 3);
        e = body; e.H = 1; chain("chain", e, SRX_OP_FWD, 0, 3); batch("batch", e, 3);
        e = body; e.N = 1; e.H = 2; chain("chain", e, SRX_OP_FWD, 0, 3); batch("batch", e, 3);
        for (int H : {204599, 204600}) { e = body; e.N = 1; e.H = H; chain("bound", e, SRX_OP_FWD, 0, 3); batch("bound", e, 3); }   // H W C 4 against 2^31 - 4096
        for (int what = 1; what <= 6; ++what) {
            chain("chain-no", body, SRX_OP_FWD, 0, 3, what);
            chain("chain-no", body, SRX_OP_BWD_DATA, R, 3, what);
        }
        for (int what = 1; what <= 5; ++what) batch("batch-no", body, 3, what);
        for (int v : {-1, 0, 1}) {
            Sw s;
            s.chain = v; chain("sw-chain", body, SRX_OP_FWD, 0, 18, 0, s);
            s = Sw(); s.chain_fixed = v; chain("sw-chain-fixed", body, SRX_OP_FWD, 0, 18, 0, s); chain("sw-chain-fixed", body, SRX_OP_BWD_DATA, R, 18, 0, s);
            s = Sw(); s.wgrad_batch = v; batch("sw-wgrad-batch", body, 18, 0, s);
        }
        for (int v : {0, 1}) { Sw s; s.conv_path = v; chain("sw-conv-path", body, SRX_OP_FWD, 0, 18, 0, s); batch("sw-conv-path", body, 18, 0, s); }
        for (int v : {-1, 0, 1, 2, 3}) { Sw s; s.wgrad_path = v; chain("sw-wgrad-path", body, SRX_OP_FWD, 0, 18, 0, s); batch("sw-wgrad-path", body, 18, 0, s); }
    }
    // ---- blocked pairs
    for (int prec : {-1, 1}) {      // (-1: srx_conv3x3_blocked_bwd_filter; 0, 1: ..._ex, which at 0 hands over to it)
        const int blocks[][2] = {{1, 1}, {2, 2}, {4, 8}, {256, 257}};
        for (auto& b : blocks) {
            blocked("blocked", 16, 32, 32, b[0], b[1], prec);
            if (b[0] == 256) continue;      // (beyond one launch's pair count: one shape is enough)
            blocked("blocked", 4, 128, 128, b[0], b[1], prec);
            blocked("blocked", 4, 64, 65, b[0], b[1], prec);
            blocked("blocked", 2, 41, 41, b[0], b[1], prec);
            blocked("blocked", 1, 5, 3, b[0], b[1], prec);
        }
        for (int W : {3, 4, 7, 8, 33, 59, 60, 67, 68}) blocked("blocked", 2, 9, W, 2, 2, prec);
        for (int W : {2047, 2048}) blocked("blocked", 1, 2048, W, 2, 2, prec);
        for (int W : {1048573, 1048574}) blocked("blocked", 1, 8, W, 2, 2, prec);
        for (int what = 1; what <= 3; ++what) blocked("blocked-no", 4, 32, 32, 2, 2, prec, what);
        blocked("blocked-no", 4, 32, 32, 0, 2, prec);
        blocked("blocked-no", 0, 32, 32, 2, 2, prec);
    }
    blocked("blocked-no", 4, 32, 32, 2, 2, 2);
    blocked("blocked", 16, 32, 32, 2, 2, 0);
    blocked("blocked", 4, 128, 128, 2, 2, 0);
    for (int v : {0, 1, 2}) { Sw s; s.wgrad_path = v; blocked("sw-wgrad-path", 16, 32, 32, 2, 2, -1, 0, s); blocked("sw-wgrad-path", 4, 128, 128, 2, 2, -1, 0, s); }
    // ---- every value of the runtime switches on the shapes whose route they change
    {
        const srx_conv_desc shapes[] = {D(64, 41, 41, 64, 64, 3, 1, SAME, R), D(2, 40, 128, 64, 64, 3, 1, SAME, R), D(1, 256, 256, 3, 64, 5, 1, SAME, TANH),
                                        D(1, 720, 1280, 64, 32, 1, 1, SAME, R), D(64, 41, 41, 64, 3, 3), D(1, 720, 1280, 32, 3, 5), D(1, 720, 1280, 32, 27, 3),
                                        D(16, 32, 32, 64, 64, 3, 2, SAME, R), D(64, 32, 32, 64, 64, 3, 1, SAME, R), D(1, 720, 1280, 3, 64, 9, 1, SAME, R)};
        for (const srx_conv_desc& d : shapes) {
            for (int v : {0, 1}) { Sw s; s.conv_path = v; all3("sw-conv-path", d, R, s); }
            for (int v : {0, 1, 2}) { Sw s; s.wgrad_path = v; wgrad("sw-wgrad-path", d, s); }
        }
    }
}

// ---- running --------------------------------------------------------------------------------------------------------
void queries(const Case& c) {
    const srx_conv_desc* d = &c.d;
    out("  workspace_bytes fwd=%zu dgrad=%zu wgrad=%zu\n", srx_conv2d_workspace_bytes(d, SRX_OP_FWD), srx_conv2d_workspace_bytes(d, SRX_OP_BWD_DATA),
        srx_conv2d_workspace_bytes(d, SRX_OP_BWD_FILTER));
    for (int op : {0, 1, 2, 3}) {
        const int ok = srx_conv2d_precision_supported(d, op);
        out("  precision_supported op=%d: %d%s%s\n", op, ok, ok ? "" : " ", ok ? "" : srx_last_error());
    }
    if (d->KH != 3 || d->Cin != 64 || d->Cout != 64) return;     // (chains and batches: the 3x3 64 -> 64 layers' business)
    for (int op : {0, 1})
        for (int ia : {0, 1}) {
            const int ok = srx_conv_chain_supported(d, op, ia);
            out("  chain_supported op=%d in_act=%d: %d%s%s\n", op, ia, ok, ok ? "" : " ", ok ? "" : srx_last_error());
        }
    for (int L : {2, 18, 32}) {
        int wpl = -1, grid = -1;
        const int rc = srx_conv2d_bwd_filter_batch_plan(d, L, &wpl, &grid);
        out("  batch_plan L=%d: rc=%d wpl=%d grid=%d ws=%zu%s%s\n", L, rc, wpl, grid, srx_conv2d_bwd_filter_batch_workspace_bytes(d, L), rc ? " " : "",
            rc ? srx_last_error() : "");
    }
}

void run_mask(const Case& c, Mode m, int hot) {
    g_mode = m; g_hot = hot; g_lines = 0; g_folded = 0; g_fold_hash = 0;
    static const char* const names[] = {"all refuse", "all accept", "launch error", "reduce error", "only"};
    out("-- %s%s%s\n", names[m], m == ONE_HOT ? " " : "", m == ONE_HOT ? srx_stub::name(hot) : "");
    int n = -1;
    const int rc = c.run(&n);
    if (g_folded) out("  ... and %ld more launcher calls, hash %016llx\n", g_folded, (unsigned long long)g_fold_hash);
    out("  rc=%d n_partials=%d err=\"%s\"\n", rc, n, rc ? srx_last_error() : "");
    if (rc) {
        std::string e = srx_last_error();
        for (char& ch : e) if (ch >= '0' && ch <= '9') ch = '#';
        g_errors.insert(e);
    }
}

const std::string& run_case(const Case& c) {
    g_text.clear();
    out("== %s\n", c.name.c_str());
    int old_path = -2;
    if (c.sw.conv_path != -2) { old_path = srx_set_conv_path(c.sw.conv_path); out("  srx_set_conv_path(%d) was %d\n", c.sw.conv_path, old_path); }
    if (c.sw.wgrad_path != -2) out("  srx_set_wgrad_path(%d) was %d\n", c.sw.wgrad_path, srx_set_wgrad_path(c.sw.wgrad_path));
    if (c.sw.chain != -2) out("  srx_set_chain(%d) was %d\n", c.sw.chain, srx_set_chain(c.sw.chain));
    if (c.sw.chain_fixed != -2) out("  srx_set_chain_fixed(%d) was %d\n", c.sw.chain_fixed, srx_set_chain_fixed(c.sw.chain_fixed));
    if (c.sw.wgrad_batch != -2) out("  srx_set_wgrad_batch(%d) was %d\n", c.sw.wgrad_batch, srx_set_wgrad_batch(c.sw.wgrad_batch));
    if (c.has_desc) queries(c);
    memset(g_offered_now, 0, sizeof(g_offered_now));
    run_mask(c, REFUSE_ALL, -1);
    bool offered[srx_stub::kIds];
    memcpy(offered, g_offered_now, sizeof(offered));
    run_mask(c, ACCEPT_ALL, -1);
    run_mask(c, ERR_LAUNCH, -1);
    run_mask(c, ERR_REDUCE, -1);
    for (int id = 0; id < srx_stub::kOffered; ++id)
        if (offered[id]) run_mask(c, ONE_HOT, id);
    // back to "not set by the caller" (the conv path has no such value: its effective value of before is the same thing)
    if (c.sw.conv_path != -2) out("  srx_set_conv_path(%d) was %d\n", old_path, srx_set_conv_path(old_path));
    if (c.sw.wgrad_path != -2) out("  srx_set_wgrad_path(-1) was %d\n", srx_set_wgrad_path(-1));
    if (c.sw.chain != -2) out("  srx_set_chain(-1) was %d\n", srx_set_chain(-1));
    if (c.sw.chain_fixed != -2) out("  srx_set_chain_fixed(-1) was %d\n", srx_set_chain_fixed(-1));
    if (c.sw.wgrad_batch != -2) out("  srx_set_wgrad_batch(-1) was %d\n", srx_set_wgrad_batch(-1));
    return g_text;
}

// every configuration: the CU counts, then one environment knob each in its non-default state
struct Config { const char* name; const char* env; };
const Config kConfigs[] = {
    {"default", "ROUTE_TRACE_CUS=256"}, {"cus24", "ROUTE_TRACE_CUS=24"},
    {"SRX_PIPE=0", "SRX_PIPE=0"}, {"SRX_NARROW=0", "SRX_NARROW=0"}, {"SRX_WGRAD_LIN=0", "SRX_WGRAD_LIN=0"}, {"SRX_WGRAD_PIPE=0", "SRX_WGRAD_PIPE=0"},
    {"SRX_WGRAD_PIPE_STRIP=0", "SRX_WGRAD_PIPE_STRIP=0"}, {"SRX_WGRAD_ROWS_FULL=0", "SRX_WGRAD_ROWS_FULL=0"}, {"SRX_WGRAD_1X1=0", "SRX_WGRAD_1X1=0"},
    {"SRX_WGRAD_PACK3=0", "SRX_WGRAD_PACK3=0"}, {"SRX_PACK3_DGRAD=0", "SRX_PACK3_DGRAD=0"}, {"SRX_STRIP_D2S=0", "SRX_STRIP_D2S=0"},
    {"SRX_CHAIN=0", "SRX_CHAIN=0"}, {"SRX_CHAIN_FIXED=0", "SRX_CHAIN_FIXED=0"}, {"SRX_WGRAD_BATCH=0", "SRX_WGRAD_BATCH=0"},
    {"SRX_KWROWS_MIN_PIXELS=-1", "SRX_KWROWS_MIN_PIXELS=-1"}, {"SRX_BIG_ROUTE_MIN_PIXELS=-1", "SRX_BIG_ROUTE_MIN_PIXELS=-1"},
    {"SRX_CONV_1X1_MIN_PIXELS=-1", "SRX_CONV_1X1_MIN_PIXELS=-1"},
};

int for_each_config(const char* self, const char* flag, const std::function<void(const Config&, const std::string&)>& f) {
    for (const Config& cfg : kConfigs) {
        const std::string cmd = std::string("env -u ROUTE_TRACE_CUS ") + cfg.env + " '" + self + "' " + flag;
        FILE* p = popen(cmd.c_str(), "r");
        if (!p) return 2;
        std::string text;
        char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), p)) > 0) text.append(buf, n);
        if (pclose(p) != 0) { fprintf(stderr, "route_trace_driver: '%s' failed\n", cmd.c_str()); return 2; }
        f(cfg, text);
    }
    return 0;
}

double now_ns() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e9 * (double)t.tv_sec + (double)t.tv_nsec;
}

int time_calls() {
    g_mode = QUIET;
    const srx_conv_desc d = D(256, 41, 41, 64, 64, 3, 1, SRX_PAD_SAME, SRX_ACT_RELU);
    const float *x[18], *w[18], *b[18];
    float* y[18];
    for (int l = 0; l < 18; ++l) { x[l] = T(LAYERS, (size_t)l << 24); w[l] = T(LAYERS + 1, (size_t)l << 24); b[l] = T(LAYERS + 2, (size_t)l << 8); y[l] = T(LAYERS + 4, (size_t)l << 24); }
    const int iters = 200000, reps = 8;
    double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {0, 0, 0};
    long bad = 0;
    for (int rep = 0; rep < reps; ++rep) {      // (the first repetition warms up)
        double t[4];
        t[0] = now_ns();
        for (int i = 0; i < iters; ++i) bad += srx_conv2d_fwd(&d, T(X), T(WT), T(BIAS), nullptr, T(Y), nullptr, 0, nullptr);
        t[1] = now_ns();
        for (int i = 0; i < iters; ++i) bad += srx_conv2d_bwd_filter(&d, T(X), T(Y), T(DW), T(DB), nullptr, 0.f, T(WS), kBigWs, nullptr);
        t[2] = now_ns();
        for (int i = 0; i < iters; ++i) bad += srx_conv_chain(&d, SRX_OP_FWD, 0, 18, x, w, b, nullptr, y, nullptr);
        t[3] = now_ns();
        for (int j = 0; j < 3 && rep; ++j) {
            const double ns = (t[j + 1] - t[j]) / iters;
            if (ns < lo[j]) lo[j] = ns;
            if (ns > hi[j]) hi[j] = ns;
        }
    }
    printf("ns per call, fastest .. slowest of %d repetitions: srx_conv2d_fwd %.1f .. %.1f  srx_conv2d_bwd_filter %.1f .. %.1f  srx_conv_chain %.1f .. %.1f\n",
           reps - 1, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
    if (bad) fprintf(stderr, "route_trace_driver --time: %ld calls failed: %s\n", bad, srx_last_error());
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string flag = argc > 1 ? argv[1] : "";
    if (flag == "--time") return time_calls();
    if (flag == "--all")
        return for_each_config(argv[0], "", [](const Config& cfg, const std::string& text) { printf("#### %s\n%s", cfg.name, text.c_str()); });
    if (flag == "--record") {
        // a case's hash: the hash of its 18 hashes, one per configuration in kConfigs' order
        std::vector<std::string> order;
        std::map<std::string, std::string> all;
        const int rc = for_each_config(argv[0], "--hashes", [&](const Config& cfg, const std::string& text) {
            size_t pos = 0;
            while (pos < text.size()) {
                size_t e = text.find('\n', pos);
                if (e == std::string::npos) e = text.size();
                const std::string line = text.substr(pos, e - pos);
                pos = e + 1;
                const size_t sp = line.find(' ');
                if (sp == std::string::npos) continue;
                const std::string name = line.substr(0, sp);
                if (!all.count(name)) order.push_back(name);
                all[name] += std::string(cfg.name) + " " + line.substr(sp + 1) + "\n";
            }
        });
        // a group: the cases of one tag and entry point ("width/wgrad"); its line holds the hash of its cases' names and
        // hashes, then the first four digits of each case's own hash, in the order of --hashes
        std::vector<std::string> groups;
        std::map<std::string, std::string> text, digits;
        for (const std::string& name : order) {
            const size_t slash = name.find('/'), end = name.find_first_of("/_+", slash + 1);
            const std::string group = name.substr(0, end);
            char hex[24];
            snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)fnv(all[name].data(), all[name].size()));
            if (!text.count(group)) groups.push_back(group);
            text[group] += name + " " + hex + "\n";
            digits[group] += std::string(" ") + std::string(hex, 4);
        }
        printf("# conv route golden: `route_trace_driver --record` (tests/test_routes_host.py).  <tag/entry point> <64-bit hash over the group's cases>:\n"
               "# <four digits of each case's hash>.  A case's hash covers its output under the %zu configurations (256 and 24 CUs, each\n"
               "# environment knob in its non-default state).\n", sizeof(kConfigs) / sizeof(kConfigs[0]));
        for (const std::string& g : groups) printf("%s %016llx:%s\n", g.c_str(), (unsigned long long)fnv(text[g].data(), text[g].size()), digits[g].c_str());
        return rc;
    }
    if (flag == "--fwd") {
        if (argc != 9) { fprintf(stderr, "route_trace_driver --fwd N H W CIN COUT K PAD\n"); return 2; }
        int v[7];
        for (int i = 0; i < 7; ++i) v[i] = atoi(argv[2 + i]);
        fwd("shape", D(v[0], v[1], v[2], v[3], v[4], v[5], 1, v[6]));
    } else {
        build_cases();
    }
    {
        std::set<std::string> names;
        for (const Case& c : g_cases)
            if (!names.insert(c.name).second) { fprintf(stderr, "route_trace_driver: case name twice: %s\n", c.name.c_str()); return 2; }
    }
    long lines = 0;
    bool found = false;
    for (const Case& c : g_cases) {
        if (flag == "--case" && (argc < 3 || c.name != argv[2])) continue;
        found = true;
        const std::string& text = run_case(c);
        for (char ch : text) lines += ch == '\n';
        if (flag == "--hashes") printf("%s %016llx\n", c.name.c_str(), (unsigned long long)fnv(text.data(), text.size()));
        else if (flag != "--coverage") fputs(text.c_str(), stdout);
    }
    if (flag == "--case" && !found) { fprintf(stderr, "route_trace_driver: no such case\n"); return 2; }
    if (flag == "--coverage") {
        printf("cases %zu lines %ld\n", g_cases.size(), lines);
        for (int id = 0; id < srx_stub::kIds; ++id)
            if (id != srx_stub::k_elementwise) printf("%s offered %ld accepted %ld\n", srx_stub::name(id), g_offered[id], g_accepted[id]);
        for (const std::string& e : g_errors) printf("error: %s\n", e.c_str());
    }
    return 0;
}
