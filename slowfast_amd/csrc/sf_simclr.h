// SimCLR NT-Xent loss on the device (slowfast/models/contrastive.py: Normalize :875-884 on both crops' features and the "simclr"
// branch of forward :692-754 -- cat, mm, exp, the off-diagonal mask, masked_select, sum, the positives, div, log, mean -- and
// their backward).  All fp32, whatever the activation type of the build; plain VALU products, no floating-point atomics: every
// sum below has one fixed order, so two runs give the same bits.
//
//   sf_simclr_norm_kernel   one wave per row of x = [a; b] (M = 2 n rows): q_r = x_r / |x_r| dense, |x_r|
//   sf_simclr_rows_kernel   a workgroup owns 16 rows i: E_ij for every j (M x M, zero on the diagonal), D_i, the row's loss term
//   sf_simclr_grad_kernel   a workgroup owns a tile of rows k: g_k from the stored E and D, the projection through the
//                           normalisation -> da / db;  ONE more workgroup: the M row terms summed -> loss
//
//   s_ij = q_i . q_j,   p(i) = (i + n) mod M,   E_ij = exp((s_ij - 1) / T) (j != i),   D_i = sum_{j != i} E_ij
//   loss = (1 / M) sum_i t_i,   t_i = (1 - s_i,p(i)) / T + log D_i
//   g_k  = sum_{j != k} E_kj (1 / D_k + 1 / D_j) q_j - 2 q_p(k),    dx_k = (1 / (M T)) (g_k - q_k (q_k . g_k)) / |x_k|
// The reference's exp(s / T) is exp(1 / T) times E: |s| <= 1, so the shift is known without a maximum pass and no exponential
// exceeds 1 for any T.  The diagonal is never formed and subtracted: E_ii is stored as 0 and D_i never sees it.
//
// E is stored, not recomputed: the gradient pass then needs no second M x M x C product, and D has the bits of the stored E.
//
// Orders.  |x_r|^2: lane l adds c = l, l + 64, ... in order, then the 6-step fold of moco_wave_sum.  s_ij: ONE accumulator over
// c = 0, 1, ... C - 1 (columns beyond C are staged as zeros), the same for (i, j) and (j, i): E is symmetric in its bits.  D_i:
// the 64 E_ij of a chunk of rows j by the 6-step fold, the chunks added in order j0 = 0, 64, ... .  g_k[c]: ONE accumulator over
// j = 0, 1, ... M - 1.  q_k . g_k: a thread adds its columns c = cg, cg + CW, ... in order, the 6-step fold per wave, then the
// waves of the row's thread group in order.  The mean: thread t of the loss workgroup adds t_t, t_{t + 256}, ... in order, then
// a halving tree over the 256 partial sums (the order of sf_byol_sim_finalize_kernel).
// No epsilon, as the reference's Normalize has none: a zero row has q = 0 / 0 = NaN, which enters every D_j through E_jr, so
// the loss and EVERY element of da and db are NaN, as there.  Nothing here selects a value with fmaxf / fminf.
#pragma once
#include "sf_moco.h"

#define SF_SIMCLR_NMAX 1024       // rows per crop (M <= 2048: the E workspace is at most 16 MiB)
#define SF_SIMCLR_CMAX 1024       // feature dimension
#define SF_SIMCLR_TI 16           // rows i per workgroup of the rows kernel (four per wave)
#define SF_SIMCLR_KC 64           // columns staged per step
#define SF_SIMCLR_RK 4            // rows k per thread of the gradient kernel

struct SimclrParams {
    const float* a;         // [n] rows lda floats apart
    const float* b;         // [n] rows ldb floats apart
    float* da;              // [n][C] dense
    float* db;              // [n][C] dense
    float* loss;            // [1]
    float* q_out;           // [n][C] dense or null: the normalised rows of a
    float* q;               // workspace [M][C]
    float* nrm;             // workspace [M]
    float* D;               // workspace [M]
    float* term;            // workspace [M]
    float* E;               // workspace [M][M]
    int n, M, C, lda, ldb;
    int cw;                 // gradient kernel: threads (= columns per pass) of one row group: 64, 128 or 256
    int ktiles;             // gradient kernel: workgroups that own rows; workgroup ktiles sums the loss
    float invT;
    float coef;             // 1 / (M T)
};

__global__ __launch_bounds__(SF_THREADS) void sf_simclr_norm_kernel(SimclrParams p) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (SF_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.M) return;
    const int C = p.C;
    const float* x = r < p.n ? p.a + (int64_t)r * p.lda : p.b + (int64_t)(r - p.n) * p.ldb;
    const float nrm = moco_row_norm(x, C, lane);
    const bool qo = p.q_out != nullptr && r < p.n;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c] / nrm;
        p.q[(int64_t)r * C + c] = v;
        if (qo) p.q_out[(int64_t)r * C + c] = v;
    }
    if (lane == 0) p.nrm[r] = nrm;
}

__global__ __launch_bounds__(SF_THREADS) void sf_simclr_rows_kernel(SimclrParams p) {
    constexpr int TI = SF_SIMCLR_TI, KC = SF_SIMCLR_KC;
    constexpr int LDT = KC + 4;                         // row pitch of sf_moco_nce_slab_kernel: a ds_read_b128 group on 16 slots
    __shared__ __attribute__((aligned(16))) float s_t[64 * LDT];
    __shared__ __attribute__((aligned(16))) float s_q[TI * LDT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int M = p.M, C = p.C, n = p.n;
    const int i0 = blockIdx.x * TI;
    float Dacc[4] = {0.f, 0.f, 0.f, 0.f}, pos[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < M; j0 += 64) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < C; c0 += KC) {
            for (int e = t; e < 64 * KC; e += SF_THREADS) {
                const int row = e / KC, c = e - row * KC;
                s_t[row * LDT + c] = (j0 + row < M && c0 + c < C) ? p.q[(int64_t)(j0 + row) * C + c0 + c] : 0.f;
            }
            for (int e = t; e < TI * KC; e += SF_THREADS) {
                const int row = e / KC, c = e - row * KC;
                s_q[row * LDT + c] = (i0 + row < M && c0 + c < C) ? p.q[(int64_t)(i0 + row) * C + c0 + c] : 0.f;
            }
            __syncthreads();
            for (int c4 = 0; c4 < KC / 4; ++c4) {
                const f32x4 tv = *reinterpret_cast<const f32x4*>(&s_t[lane * LDT + 4 * c4]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>(&s_q[(4 * w + b) * LDT + 4 * c4]);
                    d[b] += qv[0] * tv[0];
                    d[b] += qv[1] * tv[1];
                    d[b] += qv[2] * tv[2];
                    d[b] += qv[3] * tv[3];
                }
            }
            __syncthreads();
        }
        const int j = j0 + lane;
        const bool jv = j < M;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + 4 * w + b;               // wave-uniform
            const bool iv = i < M;
            const int pi = i < n ? i + n : i - n;
            const float e = (jv && j != i) ? expf((d[b] - 1.f) * p.invT) : 0.f;
            if (iv && jv) p.E[(int64_t)i * M + j] = e;
            Dacc[b] += moco_wave_sum(e);
            pos[b] += (jv && j == pi) ? d[b] : 0.f;      // one lane of one chunk holds s_i,p(i); every other term is +0
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int i = i0 + 4 * w + b;
        const float s_pos = moco_wave_sum(pos[b]);
        if (i < M && lane == 0) {
            p.D[i] = Dacc[b];
            p.term[i] = (1.f - s_pos) * p.invT + logf(Dacc[b]);
        }
    }
}

__global__ __launch_bounds__(SF_THREADS) void sf_simclr_grad_kernel(SimclrParams p) {
    constexpr int RK = SF_SIMCLR_RK;
    constexpr int TKMAX = RK * (SF_THREADS / 64);
    __shared__ float s_w[TKMAX * 64];
    __shared__ float s_rd[TKMAX];
    __shared__ float s_part[RK][SF_THREADS / 64];
    __shared__ float s_red[SF_THREADS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int M = p.M, C = p.C, n = p.n;
    if ((int)blockIdx.x == p.ktiles) {                  // the loss
        float a = 0.f;
        for (int i = t; i < M; i += SF_THREADS) a += p.term[i];
        s_red[t] = a;
        __syncthreads();
        for (int h = SF_THREADS / 2; h >= 1; h >>= 1) {
            if (t < h) s_red[t] += s_red[t + h];
            __syncthreads();
        }
        if (t == 0) p.loss[0] = s_red[0] / (float)M;
        return;
    }
    const int CW = p.cw, KG = SF_THREADS / CW, TK = RK * KG;
    const int cg = t % CW, kg = t / CW;
    const int k0 = blockIdx.x * TK;                     // rows of the workgroup: k0 .. k0 + TK - 1
    const int kb = k0 + kg * RK;                        // rows of this thread: kb .. kb + RK - 1
    if (t < TK) s_rd[t] = k0 + t < M ? 1.f / p.D[k0 + t] : 0.f;
    float acc[RK][4];
#pragma unroll
    for (int r = 0; r < RK; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[r][u] = 0.f;
    __syncthreads();
    for (int j0 = 0; j0 < M; j0 += 64) {
        for (int e = t; e < TK * 64; e += SF_THREADS) {
            const int r = e >> 6, j = j0 + (e & 63), k = k0 + r;
            s_w[e] = (k < M && j < M) ? p.E[(int64_t)k * M + j] * (s_rd[r] + 1.f / p.D[j]) : 0.f;
        }
        __syncthreads();
        const int jn = M - j0 < 64 ? M - j0 : 64;
#pragma unroll 4
        for (int jj = 0; jj < jn; ++jj) {
            const float* qj = p.q + (int64_t)(j0 + jj) * C;
            float qv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) qv[u] = cg + CW * u < C ? qj[cg + CW * u] : 0.f;
#pragma unroll
            for (int r = 0; r < RK; ++r) {
                const float wv = s_w[(kg * RK + r) * 64 + jj];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[r][u] += wv * qv[u];
            }
        }
        __syncthreads();
    }
    // g = acc - 2 q_p(k), then the partial dots q_k . g_k
    float qk[RK][4];
#pragma unroll
    for (int r = 0; r < RK; ++r) {
        const int k = kb + r;
        const bool kv = k < M;
        const int pk = k < n ? k + n : k - n;
        float dot = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg + CW * u;
            const bool v = kv && c < C;
            qk[r][u] = v ? p.q[(int64_t)k * C + c] : 0.f;
            const float qp = v ? p.q[(int64_t)pk * C + c] : 0.f;
            acc[r][u] -= 2.f * qp;
            if (!v) acc[r][u] = 0.f;
            dot += qk[r][u] * acc[r][u];
        }
        dot = moco_wave_sum(dot);
        if (lane == 0) s_part[r][w] = dot;
    }
    __syncthreads();
    const int wpg = CW / 64;                            // waves of one row group
#pragma unroll
    for (int r = 0; r < RK; ++r) {
        const int k = kb + r;
        if (k >= M) continue;
        float dot = 0.f;
        for (int x = 0; x < wpg; ++x) dot += s_part[r][kg * wpg + x];
        const float nrm = p.nrm[k];
        float* out = k < n ? p.da + (int64_t)k * C : p.db + (int64_t)(k - n) * C;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg + CW * u;
            if (c < C) out[c] = p.coef * ((acc[r][u] - qk[r][u] * dot) / nrm);
        }
    }
}
