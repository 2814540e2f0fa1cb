// Grouped 1x3x3 convolution (ResNeXt; reference call site: slowfast/models/resnet_helper.py:346-358, BottleneckTransform.b built
// with groups = num_groups) on block-diagonal MFMA tiles.
//
// A grouped convolution with Cg channels per group is a dense convolution with a block-diagonal weight.  A run of
// B = max(32, Cg) consecutive channels is a BUNDLE: conv b maps dim_inner to dim_inner, group g reads and writes channels
// [g*Cg, (g+1)*Cg), so the outputs of a bundle depend on the inputs of the same bundle only.  Per bundle the work is the
// B -> B implicit GEMM sf_igemm2.h runs for the 32- and 64-channel layers (K = 9 taps x B); the bundle index is blockIdx.y of
// sf_igemm2_kernel<.., BUNDLED = true> and offsets the channel base of the source, the packed weight, the output, the bias and
// the statistics columns, while the activations keep their pitch.  The packed operand of a bundle is [B][9*B] with zeros
// off the diagonal blocks: they cost weight bytes (8x at Cg = 4, still small beside the activations) and MFMA work nobody
// waits for -- the 1x3x3 layers are memory-bound.
//
// This header holds what the bundle scheme adds to the family: the weight packing and the weight-gradient reduction that keeps
// the diagonal blocks only.  The forward and data-gradient passes are sf_igemm2_kernel launches (sf_api.hip: gconv_launch),
// the weight-gradient partials come from the BUNDLED form of the dense weight-gradient kernels (sf_igemm.h, sf_wgrad2.h).
#pragma once
#include "sf_common.h"

// Conv3d weight [C][Cg][9] fp32 -> forward operand       wf[C][9*B]: row co, column tap*B + (ci - bundle base)
//                               -> data-gradient operand  wd[C][9*B]: row ci, column (8 - tap)*B + (co - bundle base)
// (transposed within each block, taps mirrored: the data gradient is then the forward-shaped sum over the mirrored tap order).
// Every element of both operands is written, the off-diagonal zeros included (no memset: a captured step is kernel nodes only).
struct GconvPrepParams {
    const float* w;
    f16* wf;
    f16* wd;            // may be null
    int C, Cg, B, taps;
};

__global__ __launch_bounds__(SF_THREADS) void sf_gconv_prep_kernel(GconvPrepParams p) {
    const int ld = p.taps * p.B;
    const int64_t nf = (int64_t)p.C * ld;
    const int64_t total = p.wd ? 2 * nf : nf;
    for (int64_t idx = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * SF_THREADS) {
        const bool fwd = idx < nf;
        const int64_t j = fwd ? idx : idx - nf;
        const int row = (int)(j / ld), k = (int)(j % ld);
        const int tcol = k / p.B, other = (row / p.B) * p.B + k % p.B;     // the channel on the other side, same bundle
        const int tap = fwd ? tcol : p.taps - 1 - tcol;
        const int co = fwd ? row : other, ci = fwd ? other : row;
        float v = 0.f;
        if (co / p.Cg == ci / p.Cg) v = p.w[((int64_t)co * p.Cg + ci % p.Cg) * p.taps + tap];
        (fwd ? p.wf : p.wd)[j] = (f16)v;
    }
}

// Weight gradient: per bundle the BUNDLED dense weight-gradient kernels leave `slabs` fp32 partial tile sets [Co_pad][Kpad] of the
// B x 9B product (columns tap*B + local input channel), bundle after bundle (bundle_ws floats each).  Only the diagonal blocks are
// summed -- one thread per element of dw[C][Cg][9], the slabs in a fixed order (no atomics: run-to-run identical) -- and stored:
// dw = (accumulate ? dw : 0) + out_scale * sum.  The off-diagonal products are never read.
struct GconvReduceParams {
    const float* ws;
    int slabs, Co_pad, Kpad;
    int64_t bundle_ws;
    float* dw;
    int C, Cg, B, taps;
    float out_scale;
    int accumulate;
};

__global__ __launch_bounds__(SF_THREADS) void sf_gconv_wgrad_reduce_kernel(GconvReduceParams p) {
    const int total = p.C * p.Cg * p.taps;
    const int idx = blockIdx.x * SF_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int tap = idx % p.taps, j = (idx / p.taps) % p.Cg, co = idx / (p.taps * p.Cg);
    const int bundle = co / p.B, col = co % p.B;
    const int cil = (col / p.Cg) * p.Cg + j;                    // input channel inside the bundle
    const float* src = p.ws + bundle * p.bundle_ws + (int64_t)col * p.Kpad + tap * p.B + cil;
    const int64_t slab = (int64_t)p.Co_pad * p.Kpad;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int z = 0;
    for (; z + 3 < p.slabs; z += 4) {
        a0 += src[(int64_t)z * slab];
        a1 += src[(int64_t)(z + 1) * slab];
        a2 += src[(int64_t)(z + 2) * slab];
        a3 += src[(int64_t)(z + 3) * slab];
    }
    for (; z < p.slabs; ++z) a0 += src[(int64_t)z * slab];
    const float v = ((a0 + a1) + (a2 + a3)) * p.out_scale;
    p.dw[idx] = p.accumulate ? p.dw[idx] + v : v;
}
