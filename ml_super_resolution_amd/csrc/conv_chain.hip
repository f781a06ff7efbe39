// Chained 3x3 64 -> 64 body layers: ONE persistent launch runs consecutive layers of the same pass (forward, or the data
// gradient with its ReLU-gradient mask) instead of one launch per layer.  Each workgroup keeps the row range
// conv_pipe_body gives it; the host only sends shapes where that range is whole images (N a multiple of the grid), so
// layer l + 1 of an image reads only rows that this workgroup's own waves wrote in layer l: no other workgroup is ever
// waited for.  Per layer the instruction stream is conv_pipe_body's, unchanged: every output element is the same MFMA
// sequence as in the per-layer launch, so the results are the same bits.  See DESIGN.md, "Chained body layers".
//
// Every variant exists twice: with the shape read from the arguments (GeoRuntime, any chain-eligible shape) and with the
// tile geometry of VDSR's 41 x 41 patches compiled in (Geo41), which the host picks when its plan equals those constants.
#include "launchers.h"
namespace srx {

template <bool WT, int AUX, class GEO>
__global__ __launch_bounds__(256, 1) void conv_chain_kernel(const ConvArgs a, const ChainPtrs c) {
    for (int l = 0; l < c.L; ++l) {
        ConvArgs al = a;
        al.x = c.x[l]; al.w = c.w[l]; al.bias = c.bias[l]; al.y = c.y[l];
        if (WT) al.mask = c.aux[l];
        else al.skip = c.aux[l];
        // The shape is the same for every layer, but what the body derives from it must not be hoisted out of this loop:
        // kept live across it, it would push the body's registers into spills.  Opaque copies of the fields make every
        // layer recompute it, as the per-layer launch does.  (A fixed geometry: those fields are constants, which nothing
        // can hoist into a register; only the fields it leaves to the launch are copied.)
        if constexpr (GEO::fixed) {
            asm volatile("" : "+s"(al.N), "+s"(al.units_total), "+s"(al.act), "+s"(al.post_relu), "+s"(al.mask_act));
        } else {
            asm volatile("" : "+s"(al.N), "+s"(al.H), "+s"(al.W), "+s"(al.OH), "+s"(al.OW), "+s"(al.Cin), "+s"(al.Cout));
            asm volatile("" : "+s"(al.pad_t), "+s"(al.pad_l), "+s"(al.TH), "+s"(al.TW), "+s"(al.NTX), "+s"(al.RS));
            asm volatile("" : "+s"(al.units_total), "+s"(al.act), "+s"(al.post_relu), "+s"(al.mask_act), "+s"(al.buf_floats));
        }
        // (the LDS pad columns and the address table depend on the shape only: set up once per launch)
        conv_pipe_body<3, 3, 64, 4, WT, AUX, false, GEO>(al, l == 0);
        // Layer l + 1 stages rows that the other waves of this workgroup stored in layer l: every wave waits for its
        // stores, then a workgroup-scope release / barrier / acquire (AMDGPU memory model; the waves of a workgroup
        // share the CU's vector L1).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

template <class GEO>
static hipError_t launch_chain_geo(bool wt, bool aux, const ConvArgs& a, const ChainPtrs& c, int grid, size_t lds, hipStream_t s) {
    if (!wt) return aux ? hipErrorInvalidValue : launch_with_lds<conv_chain_kernel<false, 0, GEO>>(dim3(grid), dim3(256), lds, s, a, c);
    return aux ? launch_with_lds<conv_chain_kernel<true, 1, GEO>>(dim3(grid), dim3(256), lds, s, a, c)
               : launch_with_lds<conv_chain_kernel<true, 0, GEO>>(dim3(grid), dim3(256), lds, s, a, c);
}

bool conv_chain_fixed_geometry(const ConvArgs& a, size_t lds) {
    return Geo41::matches(a) && lds == 2 * (size_t)Geo41::buf_floats * 4;
}

hipError_t launch_conv_chain(bool wt, bool aux, bool fixed, const ConvArgs& a, const ChainPtrs& c, int grid, size_t lds, hipStream_t s) {
    // the fixed instance only for a plan that equals its constants field by field; every other shape: the generic one
    if (fixed && conv_chain_fixed_geometry(a, lds)) return launch_chain_geo<Geo41>(wt, aux, a, c, grid, lds, s);
    return launch_chain_geo<GeoRuntime>(wt, aux, a, c, grid, lds, s);
}
}  // namespace srx
