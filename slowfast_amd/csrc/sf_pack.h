// Input side of the path: decoded uint8 frames -> normalised 16-bit clip in the stem's layout, one
// launch per pathway.  Replaces tensor_normalize (slowfast/datasets/utils.py:278-297: x/255, - mean, / std, in that
// order, fp32) + the THWC -> CTHW permute (datasets/kinetics.py:375-408) + pack_pathway_output's temporal
// index_select / channel reversal (datasets/utils.py:78-111):
//   out[n][to][h][w][c] = ((frames[n][t_index[to]][h][w][s] / 255) - mean[s]) / std[s],  s = c (2 - c when reversed)
// out is the N,T,H,W,4 buffer that engine.StemConvUnit reads as W pairs.
//
// ONE kernel template writes that buffer; the four entry points differ in where a pixel comes from and in the fp32 stages
// between the pixel and the single rounding to the storage type, in the reference's order (datasets/kinetics.py:402-449,
// tools/train_net.py:109-111):
//
//   entry point             SRC            ERASE  MIX    pixel -> erase -> mix -> round
//   sf_pack_clip_u8         PackDirect     -      -      the three normalised bytes
//   sf_pack_clip_u8_mix     PackDirect     -      yes    ... blended with sample N-1-n (mixup), or taken from it inside the box
//   sf_pack_clip_u8_aug     PackDirect     yes    yes    ... every sample erased by its own rows first
//   sf_pack_clip_u8_sample  PackSampled    yes    yes    ... every sample resized, cropped, flipped by its own row (sf_sample.h)
//
// Only these four are instantiated.  One thread owns one output pixel, all three channels.  value(n) = the deciding erase row's
// value for (sc, ts, y, x) of sample n, or the pixel of sample n from SRC; mixup blends value(n) with value(N-1-n) through
// mix2() (sf_mixup.h), cutmix takes value(N-1-n) inside the box, mix < 0 is no mixing.  A lane fetches a pixel only where the
// result needs it: not under an erase row, not the sample on the other side of the cutmix box edge.  A W pair (16 bytes) is
// written by two threads, so a box edge at an odd column needs no special case.  Sampling, normalisation and erasing work on
// channels in DATA.MEAN order; the channel reversal comes last.
#pragma once
#include "sf_common.h"
#include "sf_mixup.h"
#include "sf_erase.h"

struct SampleGeom {                 // sf_sample.h: sample_pixel
    const int* crop;                // device copy of the crop table
    int Hs, Ws, S;                  // padded source frame, output size
};
struct PackClipParams {
    const unsigned char* frames;    // [N][Tin][H][W][3]; sampled: [N][Tin][Hs][Ws][3]
    int N, Tin, Tout;
    int64_t HW;                     // pixels of an output plane (sampled: S * S)
    const int* t_index;             // [Tout] source frame of every output frame (null: identity)
    float mean[3], stdv[3];
    int reverse;                    // DATA.REVERSE_INPUT_CHANNEL: channel c reads source channel 2 - c
    f16* out;
    int64_t total;                  // N*Tout*HW
    FastDiv fdHW, fdT;
    FastDiv fdW;                    // plane index -> (row, column)
    int mix;                        // -1 none, 0 mixup, 1 cutmix
    float lam, oml;
    int yl, yh, xl, xh;             // cutmix box: rows yl..yh-1, columns xl..xh-1 of the output plane
    int erase_mode;
    const int* tab;                 // device copy of the erase table (sf_erase.h); null: no erasing
    const int* first_row;
    SampleGeom g;                   // sampled sources only (sf_sample.h)
};
__device__ __forceinline__ float pack_clip_norm(const unsigned char* src, int sc, const PackClipParams& p) {
    const float v = (float)src[sc] / 255.0f;
    return (v - p.mean[sc]) / p.stdv[sc];
}

// pixel source: v[sc] = normalised channel sc (DATA.MEAN order) of output pixel hw = (y, x) of source frame ts of sample n
struct PackDirect {
    static __device__ __forceinline__ void pixel(const PackClipParams& p, int n, int ts, uint32_t hw, int, int, float (&v)[3]) {
        const unsigned char* src = p.frames + (((int64_t)n * p.Tin + ts) * p.HW + hw) * 3;
#pragma unroll
        for (int sc = 0; sc < 3; ++sc) v[sc] = pack_clip_norm(src, sc, p);
    }
};

template <class SRC, bool ERASE, bool MIX>
__global__ __launch_bounds__(SF_THREADS) void sf_pack_clip_kernel(PackClipParams p) {
    for (int64_t idx = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t q, hw, n, to, y, x;
        fd_divmod((uint32_t)idx, p.fdHW, q, hw);
        fd_divmod(q, p.fdT, n, to);
        fd_divmod(hw, p.fdW, y, x);
        const int ts = p.t_index ? p.t_index[to] : (int)to;
        const int no = p.N - 1 - (int)n;
        const bool inbox = MIX && (int)y >= p.yl && (int)y < p.yh && (int)x >= p.xl && (int)x < p.xh;
        const bool need_self = !MIX || p.mix != 1 || !inbox, need_other = MIX && (p.mix == 0 || (p.mix == 1 && inbox));
        int rs = -1, ro = -1;
        if constexpr (ERASE) {
            if (p.tab && need_self) rs = erase_find(p.tab, p.first_row, (int)n, ts, (int)y, (int)x);
            if (p.tab && need_other) ro = erase_find(p.tab, p.first_row, no, ts, (int)y, (int)x);
        }
        float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
        if (need_self && rs < 0) SRC::pixel(p, (int)n, ts, hw, (int)y, (int)x, a);
        if (need_other && ro < 0) SRC::pixel(p, no, ts, hw, (int)y, (int)x, b);
        f16x4 o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = p.reverse ? 2 - c : c;           // sampling, normalisation and erasing happen before the channel reversal
            float vs = p.reverse ? a[2 - c] : a[c], vo = p.reverse ? b[2 - c] : b[c];
            if constexpr (ERASE) {
                const uint64_t e = ((uint64_t)sc * p.Tin + ts) * p.HW + hw;     // element of the normalised (3, Tin, H, W) clip
                if (rs >= 0) vs = erase_value1(p.tab, rs, p.erase_mode, 3, sc, ts, e);
                if (ro >= 0) vo = erase_value1(p.tab, ro, p.erase_mode, 3, sc, ts, e);
            }
            o[c] = (f16)(MIX && p.mix == 0 ? mix2(vs, vo, p.lam, p.oml) : (need_other ? vo : vs));
        }
        o[3] = (f16)0;
        *reinterpret_cast<f16x4*>(p.out + idx * 4) = o;
    }
}
