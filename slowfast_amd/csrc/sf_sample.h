// Spatial sampling of a training batch on the device (slowfast/datasets/utils.py:114-185 spatial_sampling, applied at
// datasets/kinetics.py:410-435 to the normalised fp32 clip: short-side scale jitter or random resized crop -- a bilinear
// F.interpolate of every frame -- then a crop and a horizontal flip).  The draw stays on the host
// (slowfast_amd/spatial_sampling.py) and arrives as ONE table with a row per sample; sample_pixel() applies it to the decoded
// uint8 frames for two sinks:
//
//   sf_sample_clip_u8       uint8 (N, T, Hs, Ws, 3) -> dense fp32 [N][3][T][S][S], the layout sf_erase_clip_f32 and
//                           sf_mix_clip_f32 work on in place (the kernel below)
//   sf_pack_clip_u8_sample  the packed path (sf_pack.h) with PackSampled as its pixel source: every sample -- and its mixing
//                           partner -- sampled through its own row, then erased and mixed in fp32, one rounding into the stems'
//                           W-pair buffer
//
// The table (int32 words, one host-to-device copy): N rows of SF_CROP_ROW_WORDS words
//     [0] src_h [1] src_w   valid size of the sample's frames inside the padded Hs x Ws buffer
//     [2] win_y [3] win_x [4] win_h [5] win_w   the source window that is resized
//     [6] res_h [7] res_w   the size the window is resized to
//     [8] off_y [9] off_x   the S x S crop inside the resized image
//     [10] flip  [11] 0
//
// Output pixel (oy, ox), per axis, in fp32 and in this order (torch's align_corners=False rule with size= given):
//     r  = o + off                          (x axis: o = S-1-ox when flip)
//     sc = (float)win_len / (float)res_len
//     f  = sc * ((float)r + 0.5f) - 0.5f;   f < 0 -> 0
//     i0 = (int)f;  l1 = f - i0;  l0 = 1 - l1;  i1 = i0 + (i0 < win_len - 1)
// taps at win_y + iy0 / iy1 and win_x + ix0 / ix1: i1 clamps to the WINDOW (the reference interpolates the cropped window, a
// byte just outside it is a wrong answer even where it exists).  Each tap is normalised exactly as sf_pack_clip_u8 does
// (pack_clip_norm), THEN blended:  l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)  -- the reference's order (it
// normalises, then interpolates), and with win_len == res_len (l1 == 0) the result is the normalised source pixel bit for
// bit.  Coordinates and blend are compiled with contraction off, so that the device and the host simulator agree.
//
// What a thread owns: one output pixel, all three channels.  The three bytes of a tap are adjacent, lanes along x read
// neighbouring (mirrored when flipped) source pixels of the same one or two source rows, so a wave's 12 byte loads per lane
// fall into a handful of cache lines and the taps that adjacent x share are served by the same lines; flip and the i1 clamp
// are arithmetic selects, never a branch.  The y coefficients cost one axis evaluation per thread (7 flops) -- less than
// exchanging them between lanes would.
#pragma once
#include "sf_common.h"
#include "sf_pack.h"

#define SF_CROP_ROW_WORDS 12

struct SampleAxis { int i0, i1; float l0, l1; };
__device__ __forceinline__ SampleAxis sample_axis(int r, int win_len, int res_len) {
#pragma clang fp contract(off)
    const float sc = (float)win_len / (float)res_len;
    float f = sc * ((float)r + 0.5f) - 0.5f;
    f = f < 0.0f ? 0.0f : f;
    SampleAxis a;
    a.i0 = (int)f;
    a.i0 = a.i0 < win_len - 1 ? a.i0 : win_len - 1;        // never taken by the rule above (f < win_len - 0.5): a bounds guard
    a.l1 = f - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    a.i1 = a.i0 + (a.i0 < win_len - 1 ? 1 : 0);
    return a;
}
__device__ __forceinline__ float sample_blend(float a, float b, float c, float d, const SampleAxis& ax, const SampleAxis& ay) {
#pragma clang fp contract(off)
    const float top = ax.l0 * a + ax.l1 * b;
    const float bot = ax.l0 * c + ax.l1 * d;
    return ay.l0 * top + ay.l1 * bot;
}

// normalised, resized, cropped, flipped value of output pixel (oy, ox) of source frame ts of sample n: channels in DATA.MEAN order
__device__ __forceinline__ void sample_pixel(const PackClipParams& p, int n, int ts, int oy, int ox, float (&v)[3]) {
    const SampleGeom& g = p.g;
    const int* c = g.crop + (int64_t)n * SF_CROP_ROW_WORDS;
    const int win_y = c[2], win_x = c[3], win_h = c[4], win_w = c[5], res_h = c[6], res_w = c[7], off_y = c[8], off_x = c[9];
    const int flip = c[10];
    const SampleAxis ay = sample_axis(oy + off_y, win_h, res_h);
    const SampleAxis ax = sample_axis((flip ? g.S - 1 - ox : ox) + off_x, win_w, res_w);
    const unsigned char* frame = p.frames + ((int64_t)n * p.Tin + ts) * g.Hs * g.Ws * 3;
    const unsigned char* r0 = frame + ((int64_t)(win_y + ay.i0) * g.Ws + win_x) * 3;
    const unsigned char* r1 = frame + ((int64_t)(win_y + ay.i1) * g.Ws + win_x) * 3;
    const int x0 = ax.i0 * 3, x1 = ax.i1 * 3;
#pragma unroll
    for (int sc = 0; sc < 3; ++sc)
        v[sc] = sample_blend(pack_clip_norm(r0 + x0, sc, p), pack_clip_norm(r0 + x1, sc, p), pack_clip_norm(r1 + x0, sc, p),
                             pack_clip_norm(r1 + x1, sc, p), ax, ay);
}

// ------------------------------------------------------------------------------------------------
// dense fp32 clip: one thread per output pixel, three stores of 4 bytes a channel plane apart (lanes along x: 256-byte runs)
struct SampleClipParams {
    PackClipParams k;           // frames, N, Tin == Tout, HW = S * S, mean / stdv, total = N * T * S * S, fdHW, fdT, fdW, g
    float* dst;                 // [N][3][T][S][S]
};
__global__ __launch_bounds__(SF_THREADS) void sf_sample_clip_u8_kernel(SampleClipParams m) {
    const PackClipParams& p = m.k;
    const int64_t plane = (int64_t)p.Tin * p.HW;
    for (int64_t idx = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t q, hw, n, t, oy, ox;
        fd_divmod((uint32_t)idx, p.fdHW, q, hw);
        fd_divmod(q, p.fdT, n, t);
        fd_divmod(hw, p.fdW, oy, ox);
        float v[3];
        sample_pixel(p, (int)n, (int)t, (int)oy, (int)ox, v);
        float* o = m.dst + ((int64_t)n * 3 * p.Tin + t) * p.HW + hw;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
    }
}

// ------------------------------------------------------------------------------------------------
// pixel source of sf_pack_clip_kernel (sf_pack.h): sample n under ITS crop row
struct PackSampled {
    static __device__ __forceinline__ void pixel(const PackClipParams& p, int n, int ts, uint32_t, int oy, int ox, float (&v)[3]) {
        sample_pixel(p, n, ts, oy, ox, v);
    }
};
