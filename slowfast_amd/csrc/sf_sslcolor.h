// SSL colour augmentation of a training batch on the device (transform.color_jitter_video_ssl, slowfast/datasets/transform.py:
// 1073-1121 with GaussianBlur at :1145-1157, applied at datasets/kinetics.py:378-387 to the decoded uint8 frames).  The draw stays
// on the host (slowfast_amd/ssl_color.py) and arrives as ONE table with a row per clip; the frames are the dense uint8
// [N][T][Hs][Ws][3] buffer of sf_u8frames.h (RGB byte order), of which sample n uses the h x w corner its row names.  The reference
// hands PIL ONE image per clip, the (T * h) x w stack of its frames: a statistic (Contrast's mean) is the clip's, and the blur's
// column passes run across the frame seams.  Inside the valid region the bytes are PIL's, bit for bit; outside it they are
// copied.
//
//   sf_sslcolor_hist_kernel        256-bin counts of L per clip, for the clips that drew contrast, after the ops drawn before it
//   sf_sslcolor_stream_kernel      brightness / contrast / saturation / hue in the drawn order and grey, per pixel
//   sf_sslcolor_blur_rows_kernel   the three box iterations along the rows of the stack, in LDS
//   sf_sslcolor_blur_cols_kernel   the three box iterations along its columns, in LDS, with a halo of 6 stacked rows
//
// The table (32-bit words): row n at n * SF_SSLCOLOR_ROW_WORDS
//     [0]      flags: 1 colour jitter, 2 grey, 4 blur, 8 grey comes BEFORE the jitter (the non-MoCo branch; after it otherwise)
//     [1]      the jitter's op order, four 4-bit fields, first op in the low bits: 0 brightness, 1 contrast, 2 saturation, 3 hue,
//              7 nothing (the op's jitter value is zero: torchvision holds None and skips it)
//     [2..4]   blend factors of brightness, contrast, saturation (float bits: the host's double rounded once, as PIL's C blend
//              receives it)
//     [5]      hue shift 0 .. 255: int(hue_factor * 255) mod 256
//     [6..8]   blur: the box's integer radius r (0 or 1: sigma <= 2), the 8.24 fixed-point weight ww of a full tap, the weight fw
//              of the two fractional taps at distance r + 1; computed on the host from sigma
//     [9],[10] h, w: the valid size of the sample's frames
//     [11..15] 0
//
// Arithmetic (PIL's observable behaviour; every floating-point expression WITHOUT contraction).  L, blend(d, v, f) and the mean of a
// 256-bin table: sf_u8frames.h.
//     brightness  blend(0, v, f);  contrast  blend(m, v, f), m the mean of L over the CLIP's T * h * w pixels;
//                 saturation  blend(L(p), v, f);  grey  (L(p), L(p), L(p))
//     hue         RGB -> HSV, H = (H + shift) & 255, HSV -> RGB
//       RGB->HSV  V = max; max == min: H = S = 0.  else in fp32: cr = max - min, s = cr / max, rc = (max - r) / cr, gc, bc alike;
//                 r == max: hh = bc - gc (fp32); else g == max: hh = (float)(2.0 + rc - bc) (fp64 sum, left to right); else
//                 hh = (float)(4.0 + gc - rc);  x = (double)hh / 6.0 + 1.0, x >= 1: x -= 1 (fmod), hh = (float)x;
//                 H = trunc((double)hh * 255.0), S = trunc((double)s * 255.0), both clipped to 0 .. 255
//       HSV->RGB  S == 0: (V, V, V).  else in fp64: hf = H * 6.0 / 255.0, i = floor(hf), f = (float)(hf - i), fs = (float)(S / 255.0),
//                 p = rnd(V * (1.0 - fs)), q = rnd(V * (1.0 - fs * f)), t = rnd(V * (1.0 - fs * (1.0 - f))), rnd(a) =
//                 floor(a + 0.5) clipped; i % 6: 0 (V,t,p)  1 (q,V,p)  2 (p,V,t)  3 (p,q,V)  4 (t,p,V)  5 (V,p,q)
//     blur        one box iteration along an axis of length n, per channel, integers only:
//                 out[x] = (ww * sum_{k=-r..r} in[clamp(x + k)] + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24,
//                 clamp to 0 .. n - 1; three iterations along the rows (n = w), then three along the columns of the stack
//                 (n = T * h: replication only at the first row of frame 0 and the last row of frame T - 1), each rounding to uint8
//
// What a thread owns.  Histogram and streaming pass: sf_u8frames.h; every op is pointwise, so the streaming pass may run in place
// (dst == src).  Row blur: a workgroup owns `rows` adjacent rows of a clip's stack (rows * 3 * w <= SF_SSLCOLOR_ROW_LDS bytes),
// SF_THREADS / rows threads walk a row byte by byte, two LDS buffers ping-pong.  Column blur: a workgroup owns SF_SSLCOLOR_COLS
// columns x SF_SSLCOLOR_RUN stacked rows plus SF_SSLCOLOR_HALO rows on either side, a thread four adjacent bytes (one dword) of a
// tile row; every iteration is computed for the whole tile with the taps clamped to the stack first and to the tile second, so
// what is wrong near the tile's edge after iteration k lies within k * (r + 1) <= 6 rows of it and never reaches the rows that are
// stored.  Clips without the pass's flag leave at once.  Histograms: the per-wave LDS counters of sf_u8frames.h, one table (L)
// per wave.
#pragma once
#include "sf_common.h"
#include "sf_u8frames.h"

#define SF_SSLCOLOR_ROW_WORDS 16
#define SF_SSLCOLOR_JITTER 1
#define SF_SSLCOLOR_GREY 2
#define SF_SSLCOLOR_BLUR 4
#define SF_SSLCOLOR_GREY_FIRST 8
#define SF_SSLCOLOR_NOP 7
#define SF_SSLCOLOR_ROW_LDS 12288       // bytes of one row-blur buffer
#define SF_SSLCOLOR_MAX_W 4096          // one row of 3 * w bytes fits the buffer
#define SF_SSLCOLOR_COLS 64             // columns of a column-blur tile
#define SF_SSLCOLOR_COLS_DW (SF_SSLCOLOR_COLS * 3 / 4)   // dwords of a tile row
#define SF_SSLCOLOR_RUN 32              // stacked rows a column-blur workgroup stores
#define SF_SSLCOLOR_HALO 6              // 3 iterations x (r + 1), r <= 1
#define SF_SSLCOLOR_TILE_ROWS (SF_SSLCOLOR_RUN + 2 * SF_SSLCOLOR_HALO)

struct SslColorParams : U8Frames {  // vec, column blur: every row of every frame is 4-byte aligned in src and dst
    const int32_t* table;       // device copy: N rows
    int* hist;                  // [N][256]: L of the clip
    int rows;                   // row blur: stacked rows per workgroup
};

// the row's jitter draws contrast
__host__ __device__ __forceinline__ bool sslcolor_needs_hist(int flags, int order) {
    if (!(flags & SF_SSLCOLOR_JITTER)) return false;
    for (int k = 0; k < 4; ++k)
        if (((order >> (4 * k)) & 15) == 1) return true;
    return false;
}

struct SslColorRow {
    int flags, order, shift;
    float fb, fc, fs;
};
__device__ __forceinline__ SslColorRow sslcolor_row(const int32_t* row) {
    SslColorRow r;
    r.flags = row[0]; r.order = row[1]; r.shift = row[5];
    r.fb = u8_f32(row[2]); r.fc = u8_f32(row[3]); r.fs = u8_f32(row[4]);
    return r;
}

__device__ __forceinline__ void sslcolor_rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
#pragma clang fp contract(off)
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    uv = maxc;
    uh = us = 0;
    if (minc == maxc) return;
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr;
    const float gc = (float)(maxc - g) / cr;
    const float bc = (float)(maxc - b) / cr;
    float hh;
    if (r == maxc) {
        hh = bc - gc;
    } else if (g == maxc) {
        const double t = 2.0 + (double)rc;
        hh = (float)(t - (double)bc);
    } else {
        const double t = 4.0 + (double)gc;
        hh = (float)(t - (double)rc);
    }
    const double sixth = (double)hh / 6.0;
    double x = sixth + 1.0;
    if (x >= 1.0) x = x - 1.0;                              // fmod(x, 1.0) of 0 <= x < 2: exact
    hh = (float)x;
    const int ih = (int)((double)hh * 255.0), is = (int)((double)s * 255.0);
    uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
    us = is < 0 ? 0 : (is > 255 ? 255 : is);
}
__device__ __forceinline__ int sslcolor_rnd(double a) {
#pragma clang fp contract(off)
    const int v = (int)floor(a + 0.5);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ void sslcolor_hsv2rgb(int h, int s, int v, int (&c)[3]) {
#pragma clang fp contract(off)
    if (s == 0) {
        c[0] = c[1] = c[2] = v;
        return;
    }
    const double h6 = (double)h * 6.0;
    const double hf = h6 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)i);
    const float fs = (float)((double)s / 255.0);
    const double vf = (double)v, dfs = (double)fs, df = (double)f;
    const double a0 = 1.0 - dfs;
    const double fsf = dfs * df;
    const double a1 = 1.0 - fsf;
    const double omf = 1.0 - df;
    const double fso = dfs * omf;
    const double a2 = 1.0 - fso;
    const double m0 = vf * a0, m1 = vf * a1, m2 = vf * a2;
    const int p = sslcolor_rnd(m0), q = sslcolor_rnd(m1), t = sslcolor_rnd(m2);
    switch (i % 6) {
        case 0: c[0] = v; c[1] = t; c[2] = p; break;
        case 1: c[0] = q; c[1] = v; c[2] = p; break;
        case 2: c[0] = p; c[1] = v; c[2] = t; break;
        case 3: c[0] = p; c[1] = q; c[2] = v; break;
        case 4: c[0] = t; c[1] = p; c[2] = v; break;
        default: c[0] = v; c[1] = p; c[2] = q; break;
    }
}
__device__ __forceinline__ void sslcolor_grey(int (&c)[3]) { c[0] = c[1] = c[2] = u8_luma(c[0], c[1], c[2]); }

// one pixel through the row.  PRE: only what precedes contrast (the histogram pass); mean: Contrast's degenerate value
template <bool PRE>
__device__ __forceinline__ void sslcolor_pixel(int (&c)[3], const SslColorRow& r, int mean) {
    if ((r.flags & (SF_SSLCOLOR_GREY | SF_SSLCOLOR_GREY_FIRST)) == (SF_SSLCOLOR_GREY | SF_SSLCOLOR_GREY_FIRST)) sslcolor_grey(c);
    if (r.flags & SF_SSLCOLOR_JITTER) {
        for (int k = 0; k < 4; ++k) {
            const int op = (r.order >> (4 * k)) & 15;
            if (op == 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = u8_blend(0, c[j], r.fb);
            } else if (op == 1) {
                if (PRE) return;
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = u8_blend(mean, c[j], r.fc);
            } else if (op == 2) {
                const int l = u8_luma(c[0], c[1], c[2]);
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = u8_blend(l, c[j], r.fs);
            } else if (op == 3) {
                int h, s, v;
                sslcolor_rgb2hsv(c[0], c[1], c[2], h, s, v);
                sslcolor_hsv2rgb((h + r.shift) & 255, s, v, c);
            }
        }
    }
    if (PRE) return;
    if ((r.flags & (SF_SSLCOLOR_GREY | SF_SSLCOLOR_GREY_FIRST)) == SF_SSLCOLOR_GREY) sslcolor_grey(c);
}

// ---- histogram of L per clip: zero grid N, count grid (chunks, N * T) -----------------------------------------------------
__global__ __launch_bounds__(SF_THREADS) void sf_sslcolor_hist_zero_kernel(SslColorParams p) {
    const int32_t* row = p.table + (int64_t)blockIdx.x * SF_SSLCOLOR_ROW_WORDS;
    if (!sslcolor_needs_hist(row[0], row[1])) return;
    p.hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = 0;
}
__global__ __launch_bounds__(SF_THREADS) void sf_sslcolor_hist_kernel(SslColorParams p) {
    __shared__ int s_h[SF_THREADS / 64][1][256];
    const int frame = blockIdx.y;
    const int n = frame / p.T;
    const int32_t* row = p.table + (int64_t)n * SF_SSLCOLOR_ROW_WORDS;
    if (!sslcolor_needs_hist(row[0], row[1])) return;       // the whole workgroup
    const SslColorRow r = sslcolor_row(row);
    const int h = row[9], w = row[10];
    if ((int)blockIdx.x * SF_U8_CHUNK >= h * p.Ws) return;  // the chunk lies below the valid rows
    u8_hist_clear(s_h);
    u8_walk<false>(p, frame, blockIdx.x, h, w, p.vec, [=](int (&c)[3], int, int) {
        sslcolor_pixel<true>(c, r, 0);
        u8_hist_count(s_h, 0, u8_luma(c[0], c[1], c[2]));
    });
    u8_hist_merge(s_h, p.hist + (int64_t)n * 256);
}

// ---- the streaming pass: grid (chunks, N * T) ------------------------------------------------------------------------------
__global__ __launch_bounds__(SF_THREADS) void sf_sslcolor_stream_kernel(SslColorParams p) {
    __shared__ int s_h[256];
    const int frame = blockIdx.y;
    const int n = frame / p.T;
    const int32_t* row = p.table + (int64_t)n * SF_SSLCOLOR_ROW_WORDS;
    const SslColorRow r = sslcolor_row(row);
    const int h = row[9], w = row[10];
    const bool work = (r.flags & (SF_SSLCOLOR_JITTER | SF_SSLCOLOR_GREY)) != 0;
    if (!work && p.dst == p.src) return;                    // in place and nothing drawn
    int mean = 0;
    if (sslcolor_needs_hist(r.flags, r.order)) {            // uniform: the whole workgroup reaches the barrier
        s_h[threadIdx.x] = p.hist[(int64_t)n * 256 + threadIdx.x];
        __syncthreads();
        mean = u8_hist_mean(s_h);                           // count > 0: h, w > 0
    }
    // nothing drawn into another buffer is a copy: an empty valid region
    u8_walk<true>(p, frame, blockIdx.x, work ? h : 0, w, p.vec, [=](int (&c)[3], int, int) { sslcolor_pixel<false>(c, r, mean); });
}

// ---- the blur -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sslcolor_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the byte of stacked row s (frame s / h, row s % h), byte column xb, of clip n
__device__ __forceinline__ int64_t sslcolor_stack_at(const SslColorParams& p, int n, int h, int s, int xb) {
    const int t = s / h, y = s - t * h;
    return (((int64_t)n * p.T + t) * p.slab + (int64_t)y * p.Ws) * 3 + xb;
}

// grid (cdiv(T * Hs, rows), N): three iterations along the rows of p.rows stacked rows; SF_THREADS / rows threads walk a row
__global__ __launch_bounds__(SF_THREADS) void sf_sslcolor_blur_rows_kernel(SslColorParams p) {
    __shared__ unsigned char s_buf[2][SF_SSLCOLOR_ROW_LDS];
    const int n = blockIdx.y;
    const int32_t* row = p.table + (int64_t)n * SF_SSLCOLOR_ROW_WORDS;
    if (!(row[0] & SF_SSLCOLOR_BLUR)) return;               // the whole workgroup
    const int rad = row[6], h = row[9], w = row[10];
    const uint32_t ww = (uint32_t)row[7], fw = (uint32_t)row[8];
    const int S = p.T * h, s0 = blockIdx.x * p.rows;
    if (s0 >= S) return;
    const int nrows = S - s0 < p.rows ? S - s0 : p.rows;
    const int wb = 3 * w;                                   // rows * wb <= rows * 3 * Ws <= SF_SSLCOLOR_ROW_LDS (the launcher checks)
    const int tpr = SF_THREADS / p.rows;                    // threads per row
    const int rr = threadIdx.x / tpr, lane = threadIdx.x - rr * tpr;
    const bool mine = rr < nrows;                           // the others only keep the barriers company
    const int64_t g0 = mine ? sslcolor_stack_at(p, n, h, s0 + rr, 0) : 0;
    if (mine)
        for (int xb = lane; xb < wb; xb += tpr) s_buf[0][rr * wb + xb] = p.src[g0 + xb];
    __syncthreads();
    for (int it = 0; it < 3; ++it) {
        const unsigned char* in = s_buf[it & 1] + rr * wb;
        unsigned char* out = s_buf[(it + 1) & 1] + rr * wb;
        if (mine)
            for (int xb = lane; xb < wb; xb += tpr) {
                const int x = xb / 3, c = xb - 3 * x;
                const unsigned char* line = in + c;
                uint32_t acc = 0;
                for (int k = -rad; k <= rad; ++k) acc += line[3 * sslcolor_clampi(x + k, 0, w - 1)];
                const uint32_t far = (uint32_t)line[3 * sslcolor_clampi(x - rad - 1, 0, w - 1)] + line[3 * sslcolor_clampi(x + rad + 1, 0, w - 1)];
                const unsigned char v = (unsigned char)((acc * ww + far * fw + (1u << 23)) >> 24);
                if (it < 2) out[xb] = v;
                else p.dst[g0 + xb] = v;
            }
        __syncthreads();
    }
}

// grid (cdiv(Ws, COLS), cdiv(T * Hs, RUN), N): three iterations along the columns of the stack.  The columns of a tile do not
// mix, so a thread owns one dword (four adjacent bytes) of a tile row: dword LDS accesses, and dword global accesses where
// p.vec says that every row of every frame starts on a 4-byte boundary (Ws % 4 == 0, aligned bases).  Tile bytes to the right of
// the valid width are loaded as they are (they lie inside the buffer: 3 * Ws is a multiple of 4 then) or as zeros, are blurred
// with everything else, and are never stored.
__global__ __launch_bounds__(SF_THREADS) void sf_sslcolor_blur_cols_kernel(SslColorParams p) {
    __shared__ uint32_t s_buf[2][SF_SSLCOLOR_TILE_ROWS][SF_SSLCOLOR_COLS_DW];
    const int n = blockIdx.z;
    const int32_t* row = p.table + (int64_t)n * SF_SSLCOLOR_ROW_WORDS;
    if (!(row[0] & SF_SSLCOLOR_BLUR)) return;               // the whole workgroup
    const int rad = row[6], h = row[9], w = row[10];
    const uint32_t ww = (uint32_t)row[7], fw = (uint32_t)row[8];
    const int S = p.T * h, s0 = blockIdx.y * SF_SSLCOLOR_RUN, x0 = blockIdx.x * SF_SSLCOLOR_COLS;
    if (s0 >= S || x0 >= w) return;
    const int wb = 3 * w, b00 = 3 * x0;                     // valid bytes of a row; the tile's first byte column
    const int sb = s0 - SF_SSLCOLOR_HALO;                                       // the stacked row of tile row 0
    const int lo = sb < 0 ? 0 : sb;                                             // the stacked rows the tile holds: lo .. hi
    const int hi = (s0 + SF_SSLCOLOR_RUN + SF_SSLCOLOR_HALO < S ? s0 + SF_SSLCOLOR_RUN + SF_SSLCOLOR_HALO : S) - 1;
    const int send = s0 + SF_SSLCOLOR_RUN < S ? s0 + SF_SSLCOLOR_RUN : S;        // rows s0 .. send - 1 are stored
    const int total = (hi - lo + 1) * SF_SSLCOLOR_COLS_DW;
    for (int i = threadIdx.x; i < total; i += SF_THREADS) {
        const int j = i / SF_SSLCOLOR_COLS_DW, d = i - j * SF_SSLCOLOR_COLS_DW;
        const int b0 = b00 + 4 * d;                         // the dword's first byte column
        uint32_t v = 0;
        if (b0 < wb) {
            const unsigned char* g = p.src + sslcolor_stack_at(p, n, h, lo + j, b0);
            if (p.vec) {
                v = *reinterpret_cast<const uint32_t*>(g);  // b0 + 4 <= 3 * Ws: both are multiples of 4
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (b0 + e < wb) v |= (uint32_t)g[e] << (8 * e);
            }
        }
        s_buf[0][lo + j - sb][d] = v;
    }
    __syncthreads();
    for (int it = 0; it < 3; ++it) {
        const uint32_t (*in)[SF_SSLCOLOR_COLS_DW] = s_buf[it & 1];
        uint32_t (*out)[SF_SSLCOLOR_COLS_DW] = s_buf[(it + 1) & 1];
        for (int i = threadIdx.x; i < total; i += SF_THREADS) {
            const int j = i / SF_SSLCOLOR_COLS_DW, d = i - j * SF_SSLCOLOR_COLS_DW;
            const int s = lo + j, b0 = b00 + 4 * d;
            if (b0 >= wb || (it == 2 && (s < s0 || s >= send))) continue;
            uint32_t acc[4] = {0, 0, 0, 0};
            // the stack's edge first (PIL's replication), the tile's second (never reached from a row that is stored)
            for (int k = -rad; k <= rad; ++k) {
                const uint32_t t = in[sslcolor_clampi(sslcolor_clampi(s + k, 0, S - 1), lo, hi) - sb][d];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (t >> (8 * e)) & 255u;
            }
            const uint32_t f0 = in[sslcolor_clampi(sslcolor_clampi(s - rad - 1, 0, S - 1), lo, hi) - sb][d];
            const uint32_t f1 = in[sslcolor_clampi(sslcolor_clampi(s + rad + 1, 0, S - 1), lo, hi) - sb][d];
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t far = ((f0 >> (8 * e)) & 255u) + ((f1 >> (8 * e)) & 255u);
                v |= ((acc[e] * ww + far * fw + (1u << 23)) >> 24) << (8 * e);
            }
            if (it < 2) {
                out[s - sb][d] = v;
                continue;
            }
            unsigned char* g = p.dst + sslcolor_stack_at(p, n, h, s, b0);
            if (p.vec && b0 + 4 <= wb) {
                *reinterpret_cast<uint32_t*>(g) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (b0 + e < wb) g[e] = (unsigned char)(v >> (8 * e));
            }
        }
        __syncthreads();
    }
}
