// The dense uint8 [N][T][Hs][Ws][3] frame buffer of sf_sample_clip_u8 (RGB byte order) and the ONE way its byte-level passes
// walk it: the histogram and streaming passes of RandAugment (sf_randaug.h) and of the SSL colour jitter (sf_sslcolor.h).  Sample
// n uses the h x w corner of its frames that its table row names; a pass changes bytes inside that region only.
//
// What a thread owns.  A frame's slab of Hs * Ws pixels is cut into chunks of SF_U8_CHUNK pixels, one workgroup each
// (grid (chunks, N * T)); the workgroup reads its sample's row, branches uniformly and hands u8_walk a pixel functor.
//   16-byte arm    16 adjacent pixels per thread -- 48 bytes, three 16-byte accesses -- when every frame slab starts on a 16-byte
//                  boundary (Hs * Ws % 16 == 0 and aligned bases: U8Frames::vec, decided by the launcher)
//   per-pixel arm  thread t takes pixels t, t + 256, ... of the chunk, so a wave's byte accesses are adjacent: otherwise, and
//                  for a functor that gathers from other pixels of src
// u8_walk guarantees, on both arms:
//   * a group of 16 pixels lies inside the slab or outside it as a whole (slab % 16 == 0 on the 16-byte arm; the per-pixel arm
//     tests every pixel), and nothing is read or written outside the slab;
//   * a thread reads all of its pixels before it writes any of them and writes no other thread's, so a pointwise functor may run
//     in place (dst == src); a functor that gathers needs dst != src;
//   * the functor sees the pixels inside the valid region only; a storing walk copies the others unchanged, and with an empty
//     valid region (h <= 0) it is a copy: the 16-byte arm then moves the words as they are.
//
// Arithmetic shared by the passes (PIL's observable behaviour; every floating-point expression WITHOUT contraction):
//     L(p)        = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16
//     blend(d,v,f): t = (float)d + f * (float)(v - d) in fp32, product rounded, then sum rounded; 0 <= f <= 1: trunc(t);
//                   otherwise t <= 0 -> 0, t >= 255 -> 255, else trunc(t)
//     mean of a 256-bin table: trunc(sum_i i * hist[i] / count + 0.5) (exact integer sums, fp64 division)
//
// Histograms: integer LDS counters, one set of C tables per wave (C KiB each) so that the four waves do not serialise on the few
// bins a natural frame fills, merged into the global table with integer atomic adds of the non-empty bins: the result does not
// depend on the order, two calls give the same bits.
#pragma once
#include "sf_common.h"

#define SF_U8_PIX 16                                // pixels per thread
#define SF_U8_CHUNK (SF_THREADS * SF_U8_PIX)        // pixels per workgroup: 4096

static_assert(SF_THREADS == 256, "a thread owns bin threadIdx.x of a 256-bin table");

typedef uint32_t u8_u32x4 __attribute__((ext_vector_type(4)));

struct U8Frames {
    const unsigned char* src;   // [N][T][Hs][Ws][3]
    unsigned char* dst;         // the same shape
    int N, T, Hs, Ws;
    int slab;                   // Hs * Ws
    int vec;                    // every frame slab is 16-byte aligned in src and dst
    FastDiv fdW;                // Ws
};

__device__ __forceinline__ int u8_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ int u8_blend(int d, int v, float f) {
#pragma clang fp contract(off)
    const float prod = f * (float)(v - d);
    const float t = (float)d + prod;
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}
__device__ __forceinline__ float u8_f32(int32_t w) {
    float f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}

// chunk `chunk` of frame `frame`: f(int (&c)[3], int x, int y) for the pixels inside the valid h x w region; STORE: the pixels
// go to dst, changed by f or as they were (a streaming pass); otherwise nothing is written (a histogram pass).  vec (uniform):
// the 16-byte arm.  No barrier inside.  f is taken by value and should capture by value ([=]): such a closure is in registers from
// the start; one that holds references keeps a row's fields in memory until the pixel loop is unrolled, and their uniform tests
// (a blend factor inside [0, 1]) are then made once per pixel, not once per workgroup.
template <bool STORE, class F>
__device__ __forceinline__ void u8_walk(const U8Frames& p, int frame, int chunk, int h, int w, bool vec, F f) {
    const unsigned char* base = p.src + (int64_t)frame * p.slab * 3;
    unsigned char* obase = STORE ? p.dst + (int64_t)frame * p.slab * 3 : nullptr;
    const int p0 = chunk * SF_U8_CHUNK;
    if (vec) {
        const int q = p0 + threadIdx.x * SF_U8_PIX;
        if (q >= p.slab) return;
        uint32_t v[12], o[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u8_u32x4 in = *reinterpret_cast<const u8_u32x4*>(base + (int64_t)q * 3 + 16 * k);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * k + e] = in[e];
        }
        if (STORE && h <= 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = v[k];
        } else {
            uint32_t y, x;
            fd_divmod((uint32_t)q, p.fdW, y, x);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
            for (int e = 0; e < SF_U8_PIX; ++e) {
                const bool in = (int)y < h && (int)x < w;
                if (STORE || in) {
                    int c[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] = (v[(3 * e + k) >> 2] >> (8 * ((3 * e + k) & 3))) & 255u;
                    if (in) f(c, (int)x, (int)y);
#pragma unroll
                    for (int k = 0; k < 3; ++k) o[(3 * e + k) >> 2] |= (uint32_t)c[k] << (8 * ((3 * e + k) & 3));
                }
                if ((int)++x == p.Ws) { x = 0; ++y; }
            }
        }
        if (STORE) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u8_u32x4 st;
#pragma unroll
                for (int e = 0; e < 4; ++e) st[e] = o[4 * k + e];
                *reinterpret_cast<u8_u32x4*>(obase + (int64_t)q * 3 + 16 * k) = st;
            }
        }
        return;
    }
#pragma nounroll                                    // 16 copies of a functor's body buy nothing and cost registers
    for (int k = 0; k < SF_U8_PIX; ++k) {
        const int q = p0 + k * SF_THREADS + threadIdx.x;
        if (q >= p.slab) break;
        uint32_t y, x;
        fd_divmod((uint32_t)q, p.fdW, y, x);
        const bool in = (int)y < h && (int)x < w;
        if (!STORE && !in) continue;
        const unsigned char* px = base + (int64_t)q * 3;
        int c[3] = {px[0], px[1], px[2]};
        if (in) f(c, (int)x, (int)y);
        if (STORE) {
            unsigned char* po = obase + (int64_t)q * 3;
            po[0] = (unsigned char)c[0];
            po[1] = (unsigned char)c[1];
            po[2] = (unsigned char)c[2];
        }
    }
}

// ---- per-wave histogram counters in LDS: C tables of 256 bins per wave ---------------------------------------------------
// clear ... count ... merge, each reached by the whole workgroup; the barriers are in clear (after) and merge (before)
template <int C>
__device__ __forceinline__ void u8_hist_clear(int (&s)[SF_THREADS / 64][C][256]) {
    for (int i = threadIdx.x; i < (SF_THREADS / 64) * C * 256; i += SF_THREADS) (&s[0][0][0])[i] = 0;
    __syncthreads();
}
template <int C>
__device__ __forceinline__ void u8_hist_count(int (&s)[SF_THREADS / 64][C][256], int c, int bin) {
    atomicAdd(&s[threadIdx.x >> 6][c][bin], 1);
}
// out: the C global tables the chunk belongs to
template <int C>
__device__ __forceinline__ void u8_hist_merge(int (&s)[SF_THREADS / 64][C][256], int* out) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int sum = 0;
#pragma unroll
        for (int wv = 0; wv < SF_THREADS / 64; ++wv) sum += s[wv][c][threadIdx.x];
        if (sum) atomicAdd(&out[c * 256 + threadIdx.x], sum);
    }
}
// Contrast's degenerate value: the mean of a 256-bin table, count > 0
__device__ __forceinline__ int u8_hist_mean(const int* hist) {
#pragma clang fp contract(off)
    int64_t sum = 0, count = 0;
    for (int k = 0; k < 256; ++k) {
        sum += (int64_t)k * hist[k];
        count += hist[k];
    }
    const double mean = (double)sum / (double)count;
    return (int)(mean + 0.5);
}
