// MaskFeat regression targets on the device: histograms of oriented gradients of the input clip, one launch
// (slowfast/models/operators.py:62-112 HOGLayerC + slowfast/models/masked.py:254-281 _get_hog_label_3d).
//
// The reference pads, runs two grouped convolutions, atan2, a scatter_add_ into a (B*T', 3, 9, H, W) fp32 tensor, two unfolds,
// a sum, a normalise and a permute / unfold / flatten chain.  sf_hog_targets_kernel reads the used frames once and writes
// the (B, T'*fs*fs, 27*u*u) targets directly in the per-token layout; gradients, bins and histograms never leave the chip.
//
// Arithmetic (fixed here).  Reflect-pad by 1.  With l_r / r_r the left / right neighbours of the three
// rows and u_c / d_c the upper / lower neighbours of the three columns of a pixel's 3x3 window,
//     gx = (l0 - r0) + 2 (l1 - r1) + (l2 - r2),        gy = (u0 - d0) + 2 (u1 - d1) + (u2 - d2):
// DIFFERENCES FIRST, so that gx (gy) is exactly 0 on a reflected border and in a flat region, as in exact arithmetic -- a
// convolution that sums the six products in another order leaves a rounding residue there, and floor(phase) then throws the
// pixel's whole magnitude into bin 8 instead of bin 0.  norm = sqrt(gx^2 + gy^2); bin = floor(atan2(gx, gy) / pi * 9) mod 9,
// taken by sign tests against the 8 inner boundary directions (k * 20 degrees) after folding the direction into the upper
// half plane: gx == 0 gives bin 0 for either sign of gy and of zero.  Cell histogram = sum of norm per bin over 8x8 pixels;
// output = histogram / max(||histogram||_2, 1e-12).
//
// Work split.  grid.z = (sample, used frame), grid.y = token row i, grid.x = chunk of nj tokens of that row.  For every
// (colour channel, cell row dh of the token) the workgroup stages the 10 x (nj*8u + 2) reflected patch in LDS -- every frame
// element is fetched once per workgroup, only the halo rows (between cell rows) and halo columns (between chunks) twice --
// then lane x of an 8-lane group owns column x of one cell: it slides a 3-row window down the 8 pixels, adds each norm into
// one of 9 register bins in row order, and the 8 lanes of the cell are folded by an xor butterfly (1, 2, 4).  The order of
// every sum is fixed: no atomics, two runs are bit-identical.  The chunk's tokens are staged in LDS and leave as ONE
// contiguous run of nj * 27*u*u floats (consecutive tokens of a row are consecutive rows of the output).  STAGE = floats of that
// LDS image: chunks of up to SF_HOG_STAGE_SMALL floats (224^2 at fs 14: 1512) take the small variant.
#pragma once
#include "sf_common.h"

#define SF_HOG_CELL 8
#define SF_HOG_BINS 9
#define SF_HOG_TILE_W 256                       // widest pixel chunk of a workgroup: one lane per pixel column
#define SF_HOG_PITCH (SF_HOG_TILE_W + 4)        // patch row pitch in floats (columns -1 .. TILE_W)
#define SF_HOG_ROWS (SF_HOG_CELL + 2)
#define SF_HOG_STAGE 8192                       // most floats of staged output per workgroup (32 KiB)
#define SF_HOG_STAGE_SMALL 2048                 // the variant for chunks that fit 8 KiB: 18.4 KiB of LDS, 8 workgroups per CU

struct HogParams {
    const float* x;         // (B, 3, T, H, W) fp32
    float* out;             // (B, Tu*fs*fs, 27*u*u) fp32
    int T, H, W;
    int ts, Tu;             // temporal stride, number of used frames
    int fs, u, nj;          // tokens per side, cells per token side, tokens per workgroup
    int F;                  // 27 * u * u
};

// sin / cos of k * 20 degrees, k = 1 .. 8
__device__ const float sf_hog_sin[8] = {0.34202014332566873f, 0.64278760968653933f, 0.86602540378443865f, 0.98480775301220806f,
                                        0.98480775301220806f, 0.86602540378443865f, 0.64278760968653933f, 0.34202014332566873f};
__device__ const float sf_hog_cos[8] = {0.93969262078590838f, 0.76604444311897804f, 0.5f, 0.17364817766693035f,
                                        -0.17364817766693035f, -0.5f, -0.76604444311897804f, -0.93969262078590838f};

__device__ __forceinline__ int hog_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// bin of the direction atan2(gx, gy): fold into gx >= 0 (theta in [0, pi)), then count the boundaries k*pi/9 at or below theta:
// sin(theta - phi_k) >= 0  <=>  gx cos(phi_k) - gy sin(phi_k) >= 0.
__device__ __forceinline__ int hog_bin(float gx, float gy) {
    if (gx == 0.f) return 0;
    if (gx < 0.f) { gx = -gx; gy = -gy; }
    int b = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) b += (gx * sf_hog_cos[k] - gy * sf_hog_sin[k] >= 0.f) ? 1 : 0;
    return b;
}

template <int STAGE>
__global__ __launch_bounds__(SF_THREADS) void sf_hog_targets_kernel(HogParams p) {
    __shared__ float patch[SF_HOG_ROWS * SF_HOG_PITCH];
    __shared__ float stage[STAGE];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * p.nj;
    const int nj = p.fs - j0 < p.nj ? p.fs - j0 : p.nj;
    const int i = blockIdx.y;
    const int b = blockIdx.z / p.Tu, t = blockIdx.z - b * p.Tu;
    const int tok_px = SF_HOG_CELL * p.u;               // pixels per token side
    const int tw = nj * tok_px;                         // pixel columns of this chunk (<= SF_HOG_TILE_W)
    const int x0 = j0 * tok_px;
    const bool active = tid < tw;
    const int cell = tid >> 3, lx = tid & 7;            // cell column inside the chunk, pixel column inside the cell
    const int jl = cell / p.u, dw = cell - jl * p.u;
    const int64_t plane = (int64_t)p.H * p.W;

    for (int c = 0; c < 3; ++c) {
        const float* frame = p.x + (((int64_t)b * 3 + c) * p.T + (int64_t)t * p.ts) * plane;
        for (int dh = 0; dh < p.u; ++dh) {
            const int y0 = (i * p.u + dh) * SF_HOG_CELL;
            __syncthreads();                            // the previous patch has been consumed
            for (int col = tid; col < tw + 2; col += SF_THREADS) {      // tw + 2 <= 258: lanes 0 and 1 take a second column
                const int xx = hog_reflect(x0 - 1 + col, p.W);
#pragma unroll
                for (int r = 0; r < SF_HOG_ROWS; ++r)
                    patch[r * SF_HOG_PITCH + col] = frame[(int64_t)hog_reflect(y0 - 1 + r, p.H) * p.W + xx];
            }
            __syncthreads();
            float h[SF_HOG_BINS];
#pragma unroll
            for (int k = 0; k < SF_HOG_BINS; ++k) h[k] = 0.f;
            if (active) {
                const float* pc = patch + tid;          // window columns tid, tid + 1, tid + 2
                float a0 = pc[0], a1 = pc[1], a2 = pc[2];
                float m0 = pc[SF_HOG_PITCH], m2 = pc[SF_HOG_PITCH + 2];
#pragma unroll
                for (int r = 0; r < SF_HOG_CELL; ++r) {
                    const float* pn = pc + (r + 2) * SF_HOG_PITCH;
                    const float n0 = pn[0], n1 = pn[1], n2 = pn[2];
                    const float gx = ((a0 - a2) + 2.f * (m0 - m2)) + (n0 - n2);
                    const float gy = ((a0 - n0) + 2.f * (a1 - n1)) + (a2 - n2);
                    const float nrm = sqrtf(gx * gx + gy * gy);
                    const int bin = hog_bin(gx, gy);
#pragma unroll
                    for (int k = 0; k < SF_HOG_BINS; ++k) h[k] += bin == k ? nrm : 0.f;
                    a0 = m0; a2 = m2;
                    a1 = pc[(r + 1) * SF_HOG_PITCH + 1];
                    m0 = n0; m2 = n2;
                }
            }
            // the 8 lanes of a cell (inactive groups carry zeros and take part in the exchange)
#pragma unroll
            for (int k = 0; k < SF_HOG_BINS; ++k) {
                h[k] += __shfl_xor(h[k], 1);
                h[k] += __shfl_xor(h[k], 2);
                h[k] += __shfl_xor(h[k], 4);
            }
            if (active) {
                float ss = 0.f;
#pragma unroll
                for (int k = 0; k < SF_HOG_BINS; ++k) ss += h[k] * h[k];
                const float den = fmaxf(sqrtf(ss), 1e-12f);
                float* dst = stage + jl * p.F + (c * SF_HOG_BINS * p.u + dh) * p.u + dw;
                const int bstride = p.u * p.u;
                // lane x writes bin x, lane 0 also bin 8
#pragma unroll
                for (int k = 0; k < SF_HOG_BINS; ++k)
                    if (lx == (k & 7) && (k < 8 || lx == 0)) dst[k * bstride] = h[k] / den;
            }
        }
    }
    __syncthreads();
    float* orow = p.out + (((int64_t)b * p.Tu + t) * p.fs * p.fs + (int64_t)i * p.fs + j0) * p.F;
    for (int e = tid; e < nj * p.F; e += SF_THREADS) orow[e] = stage[e];
}
