// MixUp / CutMix of a training batch on the device (slowfast/datasets/mixup.py; tools/train_net.py:109-111 mixes inputs[0]
// and the labels between the loader and the forward pass).  Streaming kernels, launched eagerly with scalar arguments:
//
//   sf_mix_clip_f32      the reference contract on a dense fp32 (B, C, T, H, W) clip, in place or into another buffer
//   sf_mix_targets       mixup_target(): two smoothed one-hot rows blended into a (B, K) fp32 buffer
//
// The packed uint8 path (sf_pack_clip_u8_mix and later, sf_pack.h) mixes with the mix2() of this file between the fp32
// normalisation and the 16-bit rounding.
//
// Arithmetic.  `x.mul_(lam).add_(x.flip(0).mul_(1 - lam))` is three separately rounded fp32 operations with lam and 1 - lam
// rounded to fp32 from the host's doubles; hipcc contracts a * b + c into an FMA by default, which is a different number.  Every
// blend below goes through mix2(), whose body is compiled with contraction off.
//
// In place.  Sample i is blended with sample B-1-i and vice versa, so one thread owns element e of BOTH samples of a pair:
// it loads the two values, then stores the two results.  No element is read after another thread has overwritten it, no
// temporary clip exists, and every byte is read once and written once.  The middle sample of an odd batch pairs with itself
// (mixup: fl(x*lam) + fl(x*oml), computed and stored once -- not the identity; cutmix: untouched).
#pragma once
#include "sf_common.h"

// fl(fl(a * lam) + fl(b * oml))
__device__ __forceinline__ float mix2(float a, float b, float lam, float oml) {
#pragma clang fp contract(off)
    const float pa = a * lam;
    const float pb = b * oml;
    return pa + pb;
}
__device__ __forceinline__ f32x4 mix2(f32x4 a, f32x4 b, float lam, float oml) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = mix2(a[e], b[e], lam, oml);
    return o;
}

// ------------------------------------------------------------------------------------------------
// mixup of a clip: grid.y = sample pair, grid.x strides over the S / V element groups of a sample (V = 4: 16-byte accesses,
// taken when S % 4 == 0 and both buffers are 16-byte aligned, so that every sample starts on a 16-byte boundary; V = 1
// otherwise).
struct MixClipParams {
    const float* src;
    float* dst;             // == src: in place
    int B;
    int64_t S;              // elements per sample (< 2^31)
    int H, W;               // plane geometry (cutmix)
    float lam, oml;
    int yl, yh, xl, xh;     // cutmix box: rows yl..yh-1, columns xl..xh-1 of every plane
    int vec_ok;             // 16-byte accesses are aligned (cutmix kernels)
    int g0;                 // cutmix in place: first 4-column group the box touches
    int64_t items;          // cutmix: work items per sample (pair)
    FastDiv fdG, fdR;       // item -> (row index, group) ; row index -> (plane, row)
};

template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_mixup_clip_kernel(MixClipParams p) {
    const int i = blockIdx.y, j = p.B - 1 - i;
    const int64_t n = p.S / V;
    const float* a_in = p.src + (int64_t)i * p.S;
    const float* b_in = p.src + (int64_t)j * p.S;
    float* a_out = p.dst + (int64_t)i * p.S;
    float* b_out = p.dst + (int64_t)j * p.S;
    for (int64_t e = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * SF_THREADS) {
        if constexpr (V == 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(a_in + e * 4);
            if (i == j) {
                *reinterpret_cast<f32x4*>(a_out + e * 4) = mix2(a, a, p.lam, p.oml);
            } else {
                const f32x4 b = *reinterpret_cast<const f32x4*>(b_in + e * 4);
                *reinterpret_cast<f32x4*>(a_out + e * 4) = mix2(a, b, p.lam, p.oml);
                *reinterpret_cast<f32x4*>(b_out + e * 4) = mix2(b, a, p.lam, p.oml);
            }
        } else {
            const float a = a_in[e];
            if (i == j) {
                a_out[e] = mix2(a, a, p.lam, p.oml);
            } else {
                const float b = b_in[e];
                a_out[e] = mix2(a, b, p.lam, p.oml);
                b_out[e] = mix2(b, a, p.lam, p.oml);
            }
        }
    }
}

// cutmix in place: the grid covers the BOX only.  grid.y = sample pair (i < B / 2: the middle sample of an odd batch keeps
// its pixels), one work item = one 4-column group (columns 4g .. 4g+3) of one box row of one plane.  A group that lies wholly
// inside the box is swapped with one 16-byte access per sample when the addresses allow; the groups the box edge cuts
// (odd xl / xh) and every group of a clip whose rows are not 16-byte aligned go element by element.
__global__ __launch_bounds__(SF_THREADS) void sf_cutmix_swap_kernel(MixClipParams p) {
    const int i = blockIdx.y, j = p.B - 1 - i;
    float* a = p.dst + (int64_t)i * p.S;
    float* b = p.dst + (int64_t)j * p.S;
    for (int64_t it = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; it < p.items; it += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t q, g, plane, r;
        fd_divmod((uint32_t)it, p.fdG, q, g);
        fd_divmod(q, p.fdR, plane, r);
        const int x0 = (p.g0 + (int)g) * 4;
        const int64_t row = ((int64_t)plane * p.H + p.yl + (int)r) * p.W;
        if (p.vec_ok && x0 >= p.xl && x0 + 4 <= p.xh) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(a + row + x0);
            const f32x4 vb = *reinterpret_cast<const f32x4*>(b + row + x0);
            *reinterpret_cast<f32x4*>(a + row + x0) = vb;
            *reinterpret_cast<f32x4*>(b + row + x0) = va;
        } else {
            const int xa = x0 > p.xl ? x0 : p.xl, xb = x0 + 4 < p.xh ? x0 + 4 : p.xh;
            for (int x = xa; x < xb; ++x) {
                const float va = a[row + x], vb = b[row + x];
                a[row + x] = vb;
                b[row + x] = va;
            }
        }
    }
}

// cutmix into another buffer: grid.y = sample, one work item = one 4-column group of one row of one plane;
// dst[n] = inside the box ? src[B-1-n] : src[n] (every source byte is still read once).
__global__ __launch_bounds__(SF_THREADS) void sf_cutmix_copy_kernel(MixClipParams p) {
    const int n = blockIdx.y;
    const float* self = p.src + (int64_t)n * p.S;
    const float* other = p.src + (int64_t)(p.B - 1 - n) * p.S;
    float* out = p.dst + (int64_t)n * p.S;
    for (int64_t it = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; it < p.items; it += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t q, g, plane, y;
        fd_divmod((uint32_t)it, p.fdG, q, g);
        fd_divmod(q, p.fdR, plane, y);
        const int x0 = (int)g * 4;
        const int64_t row = ((int64_t)plane * p.H + (int)y) * p.W;
        const bool yin = (int)y >= p.yl && (int)y < p.yh;
        const bool all_in = yin && x0 >= p.xl && x0 + 4 <= p.xh;
        const bool all_out = !yin || x0 + 4 <= p.xl || x0 >= p.xh;
        if (p.vec_ok && x0 + 4 <= p.W && (all_in || all_out)) {
            *reinterpret_cast<f32x4*>(out + row + x0) = *reinterpret_cast<const f32x4*>((all_in ? other : self) + row + x0);
        } else {
            const int xb = x0 + 4 < p.W ? x0 + 4 : p.W;
            for (int x = x0; x < xb; ++x) out[row + x] = ((yin && x >= p.xl && x < p.xh) ? other : self)[row + x];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// mixup_target() (slowfast/datasets/mixup.py:40-64): out[i][k] = fl(fl(v(i, k) * lam) + fl(v(B-1-i, k) * oml)) with
// v(i, k) = on when k == labels[i], off otherwise -- replaces full / scatter_ / flip / mul / add on (B, K) tensors.
struct MixTargetsParams {
    const int64_t* labels;
    int B, K;
    float on, off, lam, oml;
    float* out;
    int64_t total;
    FastDiv fdK;
};
__global__ __launch_bounds__(SF_THREADS) void sf_mix_targets_kernel(MixTargetsParams p) {
    for (int64_t idx = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t i, k;
        fd_divmod((uint32_t)idx, p.fdK, i, k);
        const float a = p.labels[i] == (int64_t)k ? p.on : p.off;
        const float b = p.labels[p.B - 1 - (int)i] == (int64_t)k ? p.on : p.off;
        p.out[idx] = mix2(a, b, p.lam, p.oml);
    }
}
