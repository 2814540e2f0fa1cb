// Colour augmentation of an AVA training batch on the device (slowfast/datasets/transform.py:268-475 color_jitter,
// lighting_jitter, color_normalization, applied at datasets/ava_dataset.py:306-333 to the [0, 1] clip after jitter, crop and
// flip, followed by the BGR -> RGB reordering).  The draw stays on the host (slowfast_amd/color_augmentation.py) and arrives as
// ONE table with a row per sample; the clip is the dense fp32 [N][3][T][HW] one that sf_sample_clip_u8 writes with mean 0 and
// std 1 (byte / 255.0f, channels in the frames' byte order: BGR for AVA, which the grey weights and the table's additions assume).
//
//   sf_color_frame_means_f32   contrast blends every frame with the mean of ITS grey values: a reduction over the frame
//   sf_color_clip_f32          everything else, in place: one streaming pass over the batch
//
// The table (32-bit words, one host-to-device copy): N rows of SF_COLOR_ROW_WORDS words
//     [0..2]   op of slot 0, 1, 2 in application order: 0 brightness, 1 contrast, 2 saturation, -1 none
//     [3]      0
//     [4 + 2s] alpha of slot s, [5 + 2s] 1 - alpha (float bits; the host takes the difference in double and rounds each once)
//     [10..12] what is added to INPUT channel 0, 1, 2 (float bits)
//     [13..15] 0
//
// Per pixel, all in fp32 without contraction and in this order:
//     gray(v)    = (0.299f * v[2] + 0.587f * v[1]) + 0.114f * v[0]
//     brightness   v[c] = v[c] * a
//     contrast     v[c] = v[c] * a + m * oma            m: the mean of gray over the frame (n, t) as the values stand there
//     saturation   g = gray(v); v[c] = v[c] * a + g * oma
//     lighting     v[c] = v[c] + add[c]
//     normalise    v[c] = (v[c] - mean[c]) / std[c]     a true division, as pack_clip_norm
//     store        out channel c = v[reverse ? 2 - c : c]
// color_until_contrast() applies the slots in front of the contrast slot; BOTH kernels call it, so the mean is taken over
// exactly the values the streaming pass blends with.
//
// What a thread owns: a pixel with all three channels (V = 4: four adjacent pixels, 16-byte accesses, taken when a frame plane
// is 16-byte aligned: HW % 4 == 0 and an aligned base; V = 1 otherwise -- planes of odd S x S are not aligned).  That makes the
// channel reversal safe in place: nobody else reads or writes the three values.
//
// The reduction is deterministic: a frame is cut into chunks of SF_COLOR_CHUNK pixels whatever the grid; one workgroup sums a
// chunk (every thread its SF_COLOR_CHUNK / SF_THREADS pixels in index order, __shfl_xor across the wave, LDS across the
// waves) and writes partials[frame][chunk]; a second launch adds a frame's partials in chunk order and divides by HW.  No
// atomics.  Frames of samples without a contrast slot are skipped by both launches and their means left untouched.
#pragma once
#include "sf_common.h"
#include "sf_pool.h"

#define SF_COLOR_ROW_WORDS 16
#define SF_COLOR_CHUNK 4096                 // pixels per workgroup of the reduction
#define SF_COLOR_MAX_CHUNKS 64              // per frame: HW <= 262144 (512 x 512)
// the longest chain of additions a grey value passes through on its way into a frame's sum: the thread's serial sum, the
// six butterfly steps of the wave, the sum over the workgroup's waves, the sum over the frame's chunks
#define SF_COLOR_SUM_DEPTH (SF_COLOR_CHUNK / SF_THREADS + 6 + (SF_THREADS / 64 - 1) + SF_COLOR_MAX_CHUNKS)

static_assert(SF_COLOR_CHUNK % (4 * SF_THREADS) == 0, "a chunk is whole 16-byte groups per thread");

struct ColorRow {
    int op[3];
    float a[3], oma[3];
    float add[3];
};
__device__ __forceinline__ ColorRow color_row(const int32_t* table, int n) {
    const int32_t* w = table + (int64_t)n * SF_COLOR_ROW_WORDS;
    const float* f = reinterpret_cast<const float*>(w);
    ColorRow r;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        r.op[s] = w[s];
        r.a[s] = f[4 + 2 * s];
        r.oma[s] = f[5 + 2 * s];
        r.add[s] = f[10 + s];
    }
    return r;
}
__device__ __forceinline__ int color_contrast_slot(const ColorRow& r) {
    return r.op[0] == 1 ? 0 : (r.op[1] == 1 ? 1 : (r.op[2] == 1 ? 2 : 3));
}
__device__ __forceinline__ float color_gray(const float (&v)[3]) {
#pragma clang fp contract(off)
    const float r = 0.299f * v[2];
    const float g = 0.587f * v[1];
    const float b = 0.114f * v[0];
    return (r + g) + b;
}
__device__ __forceinline__ float color_blend(float v, float a, float other, float oma) {
#pragma clang fp contract(off)
    const float pa = v * a;
    const float pb = other * oma;
    return pa + pb;
}
// slot s of the row on one pixel; m: the frame's grey mean (read only by a contrast slot)
__device__ __forceinline__ void color_slot(const ColorRow& r, int s, float m, float (&v)[3]) {
#pragma clang fp contract(off)
    const int op = r.op[s];
    if (op == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] * r.a[s];
    } else if (op == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = color_blend(v[c], r.a[s], m, r.oma[s]);
    } else if (op == 2) {
        const float g = color_gray(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = color_blend(v[c], r.a[s], g, r.oma[s]);
    }
}
// the slots in front of slot `upto` (the contrast slot): the values contrast takes its mean over and blends with
__device__ __forceinline__ void color_until_contrast(const ColorRow& r, int upto, float (&v)[3]) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (s < upto) color_slot(r, s, 0.0f, v);
}

struct ColorParams {
    float* clip;                // [N][3][T][HW], in place
    const int32_t* table;       // device copy
    float* partials;            // [N * T][chunks]
    float* means;               // [N * T]
    int N, T, chunks;
    int64_t HW;
    float mean[3], stdv[3];
    int reverse;
    int64_t total;              // N * T * HW / V
    FastDiv fdG, fdT;           // groups per frame, T
};

// grid (chunks, N * T); the grey value of pixel hw of frame (n, t) after the slots in front of contrast
template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_color_frame_sums_kernel(ColorParams p) {
    __shared__ float s_wave[SF_THREADS / 64];
    const int frame = blockIdx.y, n = frame / p.T, t = frame - n * p.T;
    const ColorRow r = color_row(p.table, n);
    const int upto = color_contrast_slot(r);
    if (upto == 3) return;                                  // the whole workgroup: no contrast in this sample's row
    const int64_t plane = (int64_t)p.T * p.HW;
    const float* base = p.clip + ((int64_t)n * 3 * p.T + t) * p.HW;
    const int64_t hw0 = (int64_t)blockIdx.x * SF_COLOR_CHUNK;
    float sum = 0.0f;
    for (int k = 0; k < SF_COLOR_CHUNK / (SF_THREADS * V); ++k) {
        const int64_t hw = hw0 + ((int64_t)k * SF_THREADS + threadIdx.x) * V;
        if (hw >= p.HW) break;                              // V = 4: HW % 4 == 0, a group is inside or outside as a whole
        if (V == 4) {
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(base + hw);
            const f32x4 c1 = *reinterpret_cast<const f32x4*>(base + plane + hw);
            const f32x4 c2 = *reinterpret_cast<const f32x4*>(base + 2 * plane + hw);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v[3] = {c0[e], c1[e], c2[e]};
                color_until_contrast(r, upto, v);
                sum += color_gray(v);
            }
        } else {
            float v[3] = {base[hw], base[plane + hw], base[2 * plane + hw]};
            color_until_contrast(r, upto, v);
            sum += color_gray(v);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = s_wave[0];
#pragma unroll
        for (int w = 1; w < SF_THREADS / 64; ++w) s += s_wave[w];
        p.partials[(int64_t)frame * p.chunks + blockIdx.x] = s;
    }
}
// one thread per frame: the partials in chunk order, then the division
__global__ __launch_bounds__(SF_THREADS) void sf_color_frame_means_kernel(ColorParams p) {
    const int frame = blockIdx.x * SF_THREADS + threadIdx.x;
    if (frame >= p.N * p.T) return;
    if (color_contrast_slot(color_row(p.table, frame / p.T)) == 3) return;
    const float* part = p.partials + (int64_t)frame * p.chunks;
    float s = part[0];
    for (int c = 1; c < p.chunks; ++c) s += part[c];
    p.means[frame] = s / (float)p.HW;
}

// the streaming pass: grid-strided over the N * T * HW / V pixel groups of the batch
template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_color_clip_kernel(ColorParams p) {
#pragma clang fp contract(off)
    const int64_t plane = (int64_t)p.T * p.HW;
    for (int64_t idx = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * SF_THREADS) {
        uint32_t q, g, n, t;
        fd_divmod((uint32_t)idx, p.fdG, q, g);
        fd_divmod(q, p.fdT, n, t);
        const ColorRow r = color_row(p.table, (int)n);
        const int at = color_contrast_slot(r);
        const float m = at < 3 ? p.means[q] : 0.0f;         // q = n * T + t; uniform per sample whether it is read at all
        float* base = p.clip + ((int64_t)n * 3 * p.T + t) * p.HW + (int64_t)g * V;
        float x[3][V];
        if (V == 4) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 in = *reinterpret_cast<const f32x4*>(base + c * plane);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[c][e] = in[e];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c][0] = base[c * plane];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float v[3] = {x[0][e], x[1][e], x[2][e]};
            color_until_contrast(r, at, v);
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s >= at) color_slot(r, s, m, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lit = v[c] + r.add[c];
                x[c][e] = (lit - p.mean[c]) / p.stdv[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = p.reverse ? 2 - c : c;
            if (V == 4) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = x[sc][e];
                *reinterpret_cast<f32x4*>(base + c * plane) = o;
            } else {
                base[c * plane] = x[sc][0];
            }
        }
    }
}
