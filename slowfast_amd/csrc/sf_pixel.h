// MAE regression targets on the device: the (optionally normalised) pixels of every patch of the clip, one launch
// (slowfast/models/masked.py:178-230 _patchify + _get_pixel_label_3d).
//
// The reference slices the used frames, reshapes / permutes the clip into (N, t*h*w, u*p*p*3) rows (einsum
// "nctuhpwq->nthwupqc": a strided copy of the whole clip), gathers the masked rows and takes mean, unbiased variance, a
// subtraction and a division in four more passes.  sf_pixel_targets_kernel reads every used pixel ONCE and writes the fp32
// (B, t*h*w, u*p*p*3) rows of ALL tokens directly; the dense form of the loss masks them, the gathered form indexes them.
//
// Layout.  Token (t, i, j) is row (t * h + i) * w + j, h = H / p, w = W / p, t = T / ts.  Feature ((uu * p + pp) * p + qq) * 3 + c
// is pixel (i * p + pp, j * p + qq) of colour channel c of frame t * ts + uu.  u = 1 uses frames 0, ts, 2 ts, ...
// (MASK.TIME_STRIDE_LOSS True), u = ts all of them (False).
//
// Arithmetic (fixed here).  With n = u*p*p*3 values x_i of a row, SHIFT BY THE ROW'S FIRST ELEMENT:
//     d_i = x_i - x_0,   mean_d = (sum d_i) / n,   var = (sum (d_i - mean_d)^2) / (n - 1),   out_i = (d_i - mean_d) / sqrt(var + 1e-6).
// Mean and variance are invariant under the shift in exact arithmetic; in fp32 the shift removes the row's level from every
// sum, so the summation error scales with the row's SPREAD (max |d_i|), not with its level: a constant patch (letterbox bars,
// padded frames) gives exact zeros, where sum(x) / n - x leaves a residue of |x| * 2^-24 * sqrt(n) that the division by
// sqrt(1e-6) multiplies by 1000.  Two sums per row, each two-level in a fixed order: lane l of a 64-lane wavefront adds
// elements l, l + 64, l + 128, ... serially (ceil(n / 64) terms), then the 64 partial sums are folded by an xor butterfly
// (32, 16, 8, 4, 2, 1: six steps).  Longest addition chain: ceil(n / 64) + 6 = 30 at n = 1536.  No atomics: two runs are
// bit-identical.
//
// Work split.  grid.z = (sample, token frame t), grid.y = token row i, grid.x = chunk of nj tokens of that row.  The
// workgroup copies the 3 * u * p image-row segments of nj * p contiguous floats into the LDS image of its nj output rows
// (feature stride 3 between neighbouring pixels: conflict-free), wavefront v normalises rows v, v + 4, ... in place, and
// the chunk leaves as ONE contiguous run of nj * n floats (consecutive tokens of a row are consecutive output rows).
#pragma once
#include "sf_common.h"

#define SF_PIXEL_STAGE 8192                     // floats of staged output per workgroup (32 KiB): rows of up to 8192 values

struct PixelParams {
    const float* x;         // (B, 3, T, H, W) fp32
    float* out;             // (B, t*h*w, n) fp32
    int T, H, W;
    int ts, Tt;             // temporal stride, token frames T / ts
    int u, p, h, w;         // frames per token, patch side, tokens per column / row
    int n, nj;              // row length u*p*p*3, tokens per workgroup
    int norm;
    FastDiv fdRun, fdP, fdUP;   // nj * p, p, u * p
};

__global__ __launch_bounds__(SF_THREADS) void sf_pixel_targets_kernel(PixelParams p) {
    __shared__ float stage[SF_PIXEL_STAGE];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * p.nj;
    const int nj = p.w - j0 < p.nj ? p.w - j0 : p.nj;
    const int i = blockIdx.y;
    const int b = blockIdx.z / p.Tt, t = blockIdx.z - b * p.Tt;
    const int64_t plane = (int64_t)p.H * p.W;
    const int run = nj * p.p;                               // contiguous floats of one image-row segment
    const int segs = 3 * p.u * p.p;                         // (c, uu, pp)
    const float* base = p.x + (int64_t)b * 3 * p.T * plane + (int64_t)t * p.ts * plane + (int64_t)i * p.p * p.W + j0 * p.p;
    // e walks (segment, column) with the column fastest: neighbouring lanes read neighbouring floats.  The divisor of the
    // segment split is the FULL chunk's run (p.nj * p.p) so that the magic numbers come from the host; a short last chunk skips
    // the columns it does not have.
    const int full = p.nj * p.p;
    for (int e = tid; e < segs * full; e += SF_THREADS) {
        uint32_t seg, col, c, r, uu, pp, jl, qq;
        fd_divmod((uint32_t)e, p.fdRun, seg, col);
        if ((int)col >= run) continue;
        fd_divmod(seg, p.fdUP, c, r);
        fd_divmod(r, p.fdP, uu, pp);
        fd_divmod(col, p.fdP, jl, qq);
        const float v = base[((int64_t)c * p.T + uu) * plane + (int64_t)pp * p.W + col];
        stage[jl * p.n + ((uu * p.p + pp) * p.p + qq) * 3 + c] = v;
    }
    __syncthreads();
    if (p.norm) {
        const int wave = tid >> 6, lane = tid & 63;
        for (int jl = wave; jl < nj; jl += SF_THREADS / SF_WAVE) {      // wave-uniform trip count
            float* row = stage + jl * p.n;
            const float x0 = row[0];
            float s = 0.f;
            for (int k = lane; k < p.n; k += SF_WAVE) s += row[k] - x0;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            const float mean = s / (float)p.n;
            float q = 0.f;
            for (int k = lane; k < p.n; k += SF_WAVE) {
                const float d = (row[k] - x0) - mean;
                q += d * d;
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m);
            const float den = sqrtf(q / (float)(p.n - 1) + 1.0e-6f);
            // in place: a lane rewrites only the elements it read; x0 is in a register since before the first fold, which no
            // lane passes until all 64 have reached it
            for (int k = lane; k < p.n; k += SF_WAVE) row[k] = ((row[k] - x0) - mean) / den;
        }
        __syncthreads();
    }
    float* orow = p.out + ((((int64_t)b * p.Tt + t) * p.h + i) * p.w + j0) * p.n;
    for (int e = tid; e < nj * p.n; e += SF_THREADS) orow[e] = stage[e];
}
