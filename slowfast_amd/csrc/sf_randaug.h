// RandAugment of a training batch on the device (slowfast/datasets/rand_augment.py as transform.create_random_augment calls it,
// applied at datasets/kinetics.py:389-400 to the decoded uint8 frames).  The draw stays on the host
// (slowfast_amd/rand_augment.py) and arrives as ONE table per layer with a row per sample; the frames are the dense uint8
// [N][T][Hs][Ws][3] buffer of sf_sample_clip_u8 (RGB byte order), of which sample n uses the h x w corner its row names.  Inside
// that region the bytes are PIL's, bit for bit; outside it they are copied.
//
//   sf_randaug_hist_kernel     256-bin counts of R, G, B and L per frame, for AutoContrast, Equalize and Contrast rows only
//   sf_randaug_lut_kernel      the 3 x 256 byte table of a frame, for the eight ops that are one
//   sf_randaug_stream_kernel   one layer for the whole batch: uint8 in, uint8 out
//
// The table (32-bit words, one host-to-device copy for all layers): row (layer l, sample n) at (l * N + n) * SF_RANDAUG_ROW_WORDS
//     [0]      class: 0 copy (skipped by its probability draw, or Rotate by a multiple of 360 degrees), 1 lookup table, 2 Color,
//              3 Sharpness, 4 affine gather
//     [1]      op: 0 AutoContrast, 1 Equalize, 2 Invert, 3 Rotate, 4 Posterize, 5 Solarize, 6 SolarizeAdd, 7 Color, 8 Contrast,
//              9 Brightness, 10 Sharpness, 11 ShearX, 12 ShearY, 13 TranslateXRel, 14 TranslateYRel
//     [2]      integer argument: bits kept (Posterize, 0 .. 8), threshold (Solarize, 0 .. 256), added value (SolarizeAdd)
//     [3]      blend factor f of Color, Contrast, Brightness, Sharpness (float bits: the host's double rounded once, as PIL's
//              C blend receives it)
//     [4]      filter of the affine ops: 0 bilinear, 1 bicubic
//     [5], [6] h, w: the valid size of the sample's frames
//     [7]      0
//     [8..19]  a0 .. a5 of PIL's INVERSE affine matrix for a w x h image, fp64 as (low word, high word) pairs, computed on the
//              host in Python doubles (Rotate: cos / sin of -radians(deg) rounded to 15 decimals, recentred on (w/2, h/2)); no
//              trigonometry here
//
// Arithmetic (PIL's observable behaviour; every floating-point expression WITHOUT contraction):
//     L(p), blend(d, v, f) and the mean of a 256-bin table: sf_u8frames.h
//     Brightness  blend(0, v, f)                                                          (table)
//     Color       blend(L(p), v, f) per channel
//     Contrast    blend(m, v, f), m the mean of the frame's L table                       (table)
//     Sharpness   s = (2 * acc + 13) / 26 in integers, acc the 3 x 3 sum with the centre weighted 5; the one-pixel border of
//                 the VALID region takes s = v; blend(s, v, f)
//     Invert 255 - v;  Solarize v < th ? v : 255 - v;  SolarizeAdd v < 128 ? min(255, v + add) : v;
//     Posterize   v & ~((1 << (8 - bits)) - 1), bits >= 8 the identity                    (tables)
//     AutoContrast, per channel: lo / hi the first / last non-empty bin; hi <= lo the identity; else scale = 255.0 / (hi - lo),
//                 off = -lo * scale, lut[i] = clamp(trunc(i * scale + off), 0, 255) in fp64
//     Equalize, per channel: fewer than two non-empty bins the identity; step = (count - last non-empty bin's count) / 255 in
//                 integers, 0 the identity; else n = step / 2, for i = 0 .. 255: lut[i] = min(n / step, 255), n += hist[i]
//     affine, output pixel (x, y), fp64: xin = a0*(x+0.5) + a1*(y+0.5) + a2, yin = a3*(x+0.5) + a4*(y+0.5) + a5, left to right;
//                 xin < 0 || yin < 0 || xin >= w || yin >= h: the fill (128, 128, 128), nothing is loaded; else subtract 0.5,
//                 floor and fraction, tap indices clamped to [0, w-1] / [0, h-1];
//                 bilinear  p0 + (p1 - p0) * dx per row, the same in y, trunc
//                 bicubic   PIL's transform cubic (a = -1): taps v1..v4 at x0-1 .. x0+2, p1 = v2, p2 = -v1 + v3,
//                           p3 = 2*(v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4, v = p1 + d*(p2 + d*(p3 + d*p4)), rows first,
//                           then the four row results in y; v <= 0 -> 0, v >= 255 -> 255, else trunc (NOT rounded)
//
// What a thread owns: sf_u8frames.h -- the chunks of a frame's slab, the 16-byte and the per-pixel arm, and what the walk
// guarantees.  The pointwise classes (copy, table, Color) take the 16-byte arm when the slabs are aligned; the gathering classes
// (Sharpness, affine) always take the per-pixel arm and need dst != src.  A gather fetches the adjacent taps of one row (3 x 3
// bytes for Sharpness, 2 x 3 / 4 x 3 for bilinear / bicubic) as one unaligned block when all of them lie inside the valid region,
// tap by tap with clamped columns otherwise.  Source coordinates are clamped to the valid region before every load: nothing reads
// outside the sample's slab.  Histograms: the per-wave LDS counters of sf_u8frames.h, four tables (R, G, B, L) per wave.
#pragma once
#include "sf_common.h"
#include "sf_u8frames.h"

#define SF_RANDAUG_ROW_WORDS 20
#define SF_RANDAUG_OPS 15

static_assert(SF_THREADS == 256, "the table kernel builds entry threadIdx.x of a 256-entry table");

struct RandAugParams : U8Frames {   // dst: another buffer than src
    const int32_t* table;       // device copy: the layer's N rows
    int* hist;                  // [N * T][4][256]: R, G, B, L
    unsigned char* lut;         // [N * T][3][256]
};

__host__ __device__ __forceinline__ bool randaug_needs_hist(int cls, int op) {
    return cls == 1 && (op == 0 || op == 1 || op == 8);
}
__device__ __forceinline__ double randaug_f64(const int32_t* w) {
    const uint64_t bits = (uint64_t)(uint32_t)w[0] | ((uint64_t)(uint32_t)w[1] << 32);
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}

// ---- histograms: grid (chunks, N * T) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(SF_THREADS) void sf_randaug_hist_zero_kernel(RandAugParams p) {
    const int frame = blockIdx.x;
    const int32_t* row = p.table + (int64_t)(frame / p.T) * SF_RANDAUG_ROW_WORDS;
    if (!randaug_needs_hist(row[0], row[1])) return;
    int* h = p.hist + (int64_t)frame * 1024;
#pragma unroll
    for (int c = 0; c < 4; ++c) h[c * 256 + threadIdx.x] = 0;
}
__global__ __launch_bounds__(SF_THREADS) void sf_randaug_hist_kernel(RandAugParams p) {
    __shared__ int s_h[SF_THREADS / 64][4][256];
    const int frame = blockIdx.y;
    const int32_t* row = p.table + (int64_t)(frame / p.T) * SF_RANDAUG_ROW_WORDS;
    if (!randaug_needs_hist(row[0], row[1])) return;        // the whole workgroup
    const int h = row[5], w = row[6];
    if ((int)blockIdx.x * SF_U8_CHUNK >= h * p.Ws) return;  // the chunk lies below the valid rows
    u8_hist_clear(s_h);
    u8_walk<false>(p, frame, blockIdx.x, h, w, p.vec, [=](int (&c)[3], int, int) {
        u8_hist_count(s_h, 0, c[0]);
        u8_hist_count(s_h, 1, c[1]);
        u8_hist_count(s_h, 2, c[2]);
        u8_hist_count(s_h, 3, u8_luma(c[0], c[1], c[2]));
    });
    u8_hist_merge(s_h, p.hist + (int64_t)frame * 1024);
}

// ---- lookup tables: grid N * T, thread i builds entry i of the three channels ----------------------------------------------
__global__ __launch_bounds__(SF_THREADS) void sf_randaug_lut_kernel(RandAugParams p) {
#pragma clang fp contract(off)
    __shared__ int s_h[4][256];
    const int frame = blockIdx.x;
    const int32_t* row = p.table + (int64_t)(frame / p.T) * SF_RANDAUG_ROW_WORDS;
    if (row[0] != 1) return;                                // the whole workgroup
    const int op = row[1], iarg = row[2], i = threadIdx.x;
    const float f = u8_f32(row[3]);
    int out[3] = {i, i, i};
    if (randaug_needs_hist(1, op)) {
        const int* h = p.hist + (int64_t)frame * 1024;
#pragma unroll
        for (int c = 0; c < 4; ++c) s_h[c][i] = h[c * 256 + i];
        __syncthreads();
    }
    if (op == 2) {
        out[0] = out[1] = out[2] = 255 - i;
    } else if (op == 4) {
        const int v = iarg >= 8 ? i : (i & ~((1 << (8 - iarg)) - 1));
        out[0] = out[1] = out[2] = v;
    } else if (op == 5) {
        out[0] = out[1] = out[2] = i < iarg ? i : 255 - i;
    } else if (op == 6) {
        out[0] = out[1] = out[2] = i < 128 ? (i + iarg > 255 ? 255 : i + iarg) : i;
    } else if (op == 9) {
        out[0] = out[1] = out[2] = u8_blend(0, i, f);
    } else if (op == 8) {
        out[0] = out[1] = out[2] = u8_blend(u8_hist_mean(s_h[3]), i, f);
    } else if (op == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int lo = 256, hi = -1;
            for (int k = 0; k < 256; ++k)
                if (s_h[c][k]) {
                    if (lo == 256) lo = k;
                    hi = k;
                }
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double off = (double)(-lo) * scale;
                const double prod = (double)i * scale;
                const int v = (int)(prod + off);
                out[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
            }
        }
    } else if (op == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int64_t total = 0, below = 0;
            int nz = 0, last = 0;
            for (int k = 0; k < 256; ++k) {
                const int hk = s_h[c][k];
                if (hk) {
                    ++nz;
                    last = hk;
                }
                total += hk;
                if (k < i) below += hk;
            }
            const int64_t step = (total - last) / 255;
            if (nz > 1 && step > 0) {
                const int64_t v = (step / 2 + below) / step;
                out[c] = (int)(v > 255 ? 255 : v);
            }
        }
    }
    unsigned char* lut = p.lut + (int64_t)frame * 768;
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + i] = (unsigned char)out[c];
}

// ---- the streaming pass ----------------------------------------------------------------------------------------------------
// the byte of channel c at (x, y) of the frame, x / y clamped to the valid region
__device__ __forceinline__ int randaug_tap(const unsigned char* base, int Ws, int w, int h, int x, int y, int c) {
    x = x < 0 ? 0 : (x < w ? x : w - 1);
    y = y < 0 ? 0 : (y < h ? y : h - 1);
    return base[((int64_t)y * Ws + x) * 3 + c];
}
__device__ __forceinline__ double randaug_cubic(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    const double t4 = d * p4;
    const double s3 = p3 + t4;
    const double t3 = d * s3;
    const double s2 = p2 + t3;
    const double t2 = d * s2;
    return p1 + t2;
}
__device__ __forceinline__ double randaug_lerp(double a, double b, double d) {
#pragma clang fp contract(off)
    const double diff = b - a;
    const double prod = diff * d;
    return a + prod;
}
// K adjacent pixels of row y starting at column x0, all inside the valid region: 3 * K adjacent bytes, fetched as one unaligned
// block (dword loads) instead of 3 * K byte loads; t[j][c] = channel c of pixel x0 + j
template <int K>
__device__ __forceinline__ void randaug_run(const unsigned char* base, int Ws, int x0, int y, int (&t)[K][3]) {
    unsigned char b[3 * K];
    __builtin_memcpy(b, base + ((int64_t)y * Ws + x0) * 3, 3 * K);
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[j][c] = b[3 * j + c];
}
// the same with every column clamped to the valid region (the slow path at the left / right edge)
template <int K>
__device__ __forceinline__ void randaug_run_clamped(const unsigned char* base, int Ws, int w, int h, int x0, int y, int (&t)[K][3]) {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[j][c] = randaug_tap(base, Ws, w, h, x0 + j, y, c);
}
// Sharpness at (x, y) of the valid region; in: the pixel itself
__device__ __forceinline__ void randaug_sharpness(const unsigned char* base, int Ws, int w, int h, int x, int y, float f,
                                                  const int (&in)[3], int (&out)[3]) {
    const bool border = x == 0 || y == 0 || x == w - 1 || y == h - 1;
    int acc[3] = {4 * in[0], 4 * in[1], 4 * in[2]};
    if (!border) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            int t[3][3];
            randaug_run<3>(base, Ws, x - 1, y + dy, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += t[0][c] + t[1][c] + t[2][c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = u8_blend(border ? in[c] : (2 * acc[c] + 13) / 26, in[c], f);
}
// the affine gather at output pixel (x, y) of the valid region
__device__ __forceinline__ void randaug_affine(const unsigned char* base, int Ws, int w, int h, int x, int y, const double (&a)[6],
                                               int filter, int (&out)[3]) {
#pragma clang fp contract(off)
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    const double x0 = a[0] * xc, x1 = a[1] * yc;
    const double y0 = a[3] * xc, y1 = a[4] * yc;
    double xin = (x0 + x1) + a[2];
    double yin = (y0 + y1) + a[5];
    out[0] = out[1] = out[2] = 128;
    if (!(xin >= 0.0 && yin >= 0.0 && xin < (double)w && yin < (double)h)) return;     // NaN cannot arise: the host checks
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const int ix = (int)fx, iy = (int)fy;                   // -1 .. w - 1, -1 .. h - 1
    const double dx = xin - fx, dy = yin - fy;
    if (filter == 0) {
        const bool inner = ix >= 0 && ix + 1 <= w - 1;
        double r[2][3];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int yy = iy + k < 0 ? 0 : (iy + k < h ? iy + k : h - 1);
            int t[2][3];
            if (inner) randaug_run<2>(base, Ws, ix, yy, t);
            else randaug_run_clamped<2>(base, Ws, w, h, ix, yy, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) r[k][c] = randaug_lerp((double)t[0][c], (double)t[1][c], dx);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (int)randaug_lerp(r[0][c], r[1][c], dy);
    } else {
        const bool inner = ix >= 1 && ix + 2 <= w - 1;
        double r[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = iy - 1 + k < 0 ? 0 : (iy - 1 + k < h ? iy - 1 + k : h - 1);
            int t[4][3];
            if (inner) randaug_run<4>(base, Ws, ix - 1, yy, t);
            else randaug_run_clamped<4>(base, Ws, w, h, ix - 1, yy, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) r[k][c] = randaug_cubic((double)t[0][c], (double)t[1][c], (double)t[2][c], (double)t[3][c], dx);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = randaug_cubic(r[0][c], r[1][c], r[2][c], r[3][c], dy);
            out[c] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v);
        }
    }
}

// grid (chunks, N * T)
__global__ __launch_bounds__(SF_THREADS) void sf_randaug_stream_kernel(RandAugParams p) {
    __shared__ unsigned char s_lut[768];
    const int frame = blockIdx.y;
    const int32_t* row = p.table + (int64_t)(frame / p.T) * SF_RANDAUG_ROW_WORDS;
    const int cls = row[0], h = row[5], w = row[6];
    const float f = u8_f32(row[3]);
    if (cls == 1) {                                         // uniform: the whole workgroup reaches the barrier
        const unsigned char* lut = p.lut + (int64_t)frame * 768;
        for (int i = threadIdx.x; i < 768; i += SF_THREADS) s_lut[i] = lut[i];
        __syncthreads();
    }
    if (cls <= 2) {                                         // pointwise; class 0 is a copy: an empty valid region
        u8_walk<true>(p, frame, blockIdx.x, cls == 0 ? 0 : h, w, p.vec, [=](int (&c)[3], int, int) {
            if (cls == 1) {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = s_lut[k * 256 + c[k]];
            } else {
                const int l = u8_luma(c[0], c[1], c[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = u8_blend(l, c[k], f);
            }
        });
        return;
    }
    // Sharpness and the affine ops (class 4: the launcher admits 0 .. 4) gather from their neighbours in src: the per-pixel arm,
    // dst != src (the launcher checks).  A walk per class: one loop around both gathers costs the kernel a wave per SIMD.
    const unsigned char* base = p.src + (int64_t)frame * p.slab * 3;
    if (cls == 3) {
        u8_walk<true>(p, frame, blockIdx.x, h, w, false, [=](int (&c)[3], int x, int y) {
            const int in[3] = {c[0], c[1], c[2]};
            randaug_sharpness(base, p.Ws, w, h, x, y, f, in, c);
        });
        return;
    }
    double a[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = randaug_f64(row + 8 + 2 * k);
    const int filter = row[4];
    u8_walk<true>(p, frame, blockIdx.x, h, w, false,
                  [=](int (&c)[3], int x, int y) { randaug_affine(base, p.Ws, w, h, x, y, a, filter, c); });
}
