// BYOL similarity loss on the device (slowfast/models/contrastive.py: Normalize :875-884 on the predictor output, sim_loss
// :237-243 and its loop over the keys in the "byol" branch of forward :531-535, and their backward).  All fp32, whatever the
// activation type of the build; no floating-point atomics: every sum below has one fixed order, so two runs give the same bits.
//
//   sf_byol_sim_rows_kernel      one wave per row i: q_i = p_i / |p_i|, the V similarities, the row's loss term, df_i
//   sf_byol_sim_finalize_kernel  ONE workgroup: the n row terms summed in a fixed order -> loss
//
//   loss = sum_v [ -mean_i((q_i . key_v,i) / T) ] / V
//   df_i = -(1 / (V n T)) (S_i - q_i (q_i . S_i)) / |p_i|,   S_i = sum_v key_v,i      (d loss / d p_i, through the normalisation)
//
// Orders.  A C-term dot: lane l adds c = l, l + 64, ... in order, then the 6-step fold of moco_wave_sum.  The view sums (the
// row's loss term t_i = sum_v s_v,i / T and S_i[c]) run v = 0, 1, ... .  The mean: thread t of the one finalize workgroup adds
// t_t, t_{t + 256}, ... in order, then a halving tree over the 256 partial sums.
// No epsilon, as the reference's Normalize has none: a zero row has q = 0 / 0 = NaN, which reaches its df and the loss only.
// The row is short (C <= 4096, 1 KiB per lane-strided pass at the recipe's C = 256) and is re-read from the cache by each of
// the passes instead of being kept in registers: one code path for every C.
#pragma once
#include "sf_moco.h"

#define SF_BYOL_VMAX 16           // key views per call
#define SF_BYOL_CMAX 4096         // feature dimension

struct ByolSimParams {
    const float* p;         // [n][ld] raw predictor output
    const float* key;       // [V][n][C] normalised keys, dense
    float* df;              // [n][C] dense
    float* loss;            // [1]
    float* ws;              // [n] row terms
    int n, V, C, ld;
    float invT;
    float coef;             // -(1 / T) / (V n)
};

__global__ __launch_bounds__(SF_THREADS) void sf_byol_sim_rows_kernel(ByolSimParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (SF_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (i >= p.n) return;
    const int C = p.C;
    const float* x = p.p + (int64_t)i * p.ld;
    const float* k0 = p.key + (int64_t)i * C;
    const int64_t kv = (int64_t)p.n * C;                                     // floats from one view's row i to the next view's
    const float nrm = moco_row_norm(x, C, lane);
    float term = 0.f;
    for (int v = 0; v < p.V; ++v) {
        const float* kr = k0 + v * kv;
        float d = 0.f;
        for (int c = lane; c < C; c += 64) d += (x[c] / nrm) * kr[c];
        term += moco_wave_sum(d) * p.invT;
    }
    if (lane == 0) p.ws[i] = term;
    float ds = 0.f;
    for (int c = lane; c < C; c += 64) {
        float S = 0.f;
        for (int v = 0; v < p.V; ++v) S += k0[v * kv + c];
        ds += (x[c] / nrm) * S;
    }
    const float dot = moco_wave_sum(ds);                                     // q_i . S_i
    for (int c = lane; c < C; c += 64) {
        float S = 0.f;
        for (int v = 0; v < p.V; ++v) S += k0[v * kv + c];                   // the bits of the pass above
        p.df[(int64_t)i * C + c] = p.coef * ((S - (x[c] / nrm) * dot) / nrm);
    }
}

__global__ __launch_bounds__(SF_THREADS) void sf_byol_sim_finalize_kernel(ByolSimParams p) {
    __shared__ float s_red[SF_THREADS];
    const int t = threadIdx.x;
    float a = 0.f;
    for (int64_t i = t; i < p.n; i += SF_THREADS) a += p.ws[i];
    s_red[t] = a;
    __syncthreads();
    for (int h = SF_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) s_red[t] += s_red[t + h];
        __syncthreads();
    }
    if (t == 0) p.loss[0] = -s_red[0] / ((float)p.n * (float)p.V);
}
