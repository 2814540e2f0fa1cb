// MoCo step glue on the device (slowfast/models/contrastive.py: Normalize :875-884, the "moco" branch of forward :443-483,
// _dequeue_and_enqueue :255-281, _update_history :153-166).  All fp32, whatever the activation type of the build; no
// floating-point atomics: every sum below has one fixed order, so two runs give the same bits.
//
//   sf_l2norm_rows_kernel        out[r] = x[s] / sqrt(sum_c x[s][c]^2), s = perm ? perm[r] : r   (Normalize + _batch_unshuffle)
//   sf_moco_nce_slab_kernel      one workgroup = one slab of queue rows: negatives' logits, online-softmax partials
//   sf_moco_nce_finalize_kernel  one workgroup per query row: positives, lse, df; one more workgroup: the loss
//   sf_queue_enqueue_kernel      the key queue's ring write, pointer and error word in device memory
//   sf_ema_update_kernel         hist = fl(fl(p * (1 - m)) + fl(hist * m)), (m, 1 - m) read from device memory
//
// No epsilon anywhere in the normalisation, as the reference's Normalize has none: a zero row gives NaN (0 / 0), as it does
// there.
//
// The fused loss.  The reference builds logits = cat_v([q . key_v, q . queue^T]) / T and hands it to CrossEntropyLoss with
// target 0; forward and backward read the queue and the (V n) x (1 + K) probabilities several times over.  Here the queue is
// read ONCE: a workgroup normalises f to q in LDS (n C <= 8192 floats), stages 64 queue rows at a time, writes
// l[i][j] = (q_i . queue_j) / T to the V row blocks of the logits (the negatives do not depend on the view) and keeps, per
// query row i, the running maximum M, S = sum_j exp(l_ij - M) and A[c] = sum_j exp(l_ij - M) queue_j[c], rescaled when the
// maximum moves.  The gradient of the loss w.r.t. q_i needs nothing else of the queue:
//     dq_i = 1 / (R T) sum_v [(p_v,i,0 - 1) key_v,i + exp(M_i - lse_v,i) A_i],     R = V n,
// which the finalize kernel pushes through the normalisation, df_i = (dq_i - q_i (q_i . dq_i)) / |f_i|.
#pragma once
#include "sf_common.h"

#define SF_MOCO_CHUNK 64          // queue rows staged per step (one per lane of a wave)
#define SF_MOCO_QMAX 8192         // n * C floats of q kept in LDS
#define SF_MOCO_VMAX 16           // key views per call
#define SF_MOCO_SLABS 256         // at most this many slabs (one per CU)

__device__ __forceinline__ float moco_wave_sum(float v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float moco_wave_max(float v) {
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
// |x| of one row by one wave: lane l sums c = l, l + 64, ... in order, then the 6-step fold; every lane returns the norm
__device__ __forceinline__ float moco_row_norm(const float* x, int C, int lane) {
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) ss += x[c] * x[c];
    return sqrtf(moco_wave_sum(ss));
}

// ------------------------------------------------------------------------------------------------
struct L2NormParams {
    const float* x;
    const int32_t* perm;    // or null
    float* out;             // dense [n][C]
    int n, C, ld;
};
__global__ __launch_bounds__(SF_THREADS) void sf_l2norm_rows_kernel(L2NormParams p) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (SF_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.n) return;
    const int s = p.perm ? p.perm[r] : r;                                    // validated by the host: 0 <= s < n
    const float* x = p.x + (int64_t)s * p.ld;
    const float nrm = moco_row_norm(x, p.C, lane);
    for (int c = lane; c < p.C; c += 64) p.out[(int64_t)r * p.C + c] = x[c] / nrm;
}

// ------------------------------------------------------------------------------------------------
struct MocoNceParams {
    const float* f;         // [n][C] raw query features
    const float* key;       // [V][n][C] normalised keys
    const float* queue;     // [K][C], 16-byte aligned
    float* logits;          // [V n][1 + K]
    float* ws_ms;           // [nslab][n][2]: M, S
    float* ws_a;            // [nslab][n][C], 16-byte aligned
    float* df;              // [n][C]
    float* loss;            // [1]
    int n, V, K, C;
    int slab_rows, nslab;
    float invT;
};

template <int C>
__global__ __launch_bounds__(SF_THREADS) void sf_moco_nce_slab_kernel(MocoNceParams p) {
    constexpr int LDT = C + 4;                          // staged queue row pitch: 16 lanes of a ds_read_b128 group on 16 slots
    constexpr int LDE = SF_MOCO_CHUNK + 4;
    constexpr int C4 = C / 4;
    constexpr int IG = SF_THREADS / C4;                 // query-row groups of the A update
    constexpr int NMAX = SF_MOCO_QMAX / C;
    constexpr int RP = (NMAX + IG - 1) / IG;            // query rows per thread in the A update
    constexpr int PF = C / 16;                          // 16-byte pieces of a staged chunk per thread
    __shared__ __attribute__((aligned(16))) float s_q[SF_MOCO_QMAX];
    __shared__ __attribute__((aligned(16))) float s_t[SF_MOCO_CHUNK * LDT];
    __shared__ __attribute__((aligned(16))) float s_e[NMAX * LDE];
    __shared__ float s_m[NMAX], s_s[NMAX], s_al[NMAX];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = p.n;
    const int64_t ldl = (int64_t)p.K + 1;
    for (int i = w; i < n; i += SF_THREADS / 64) {
        const float* fr = p.f + (int64_t)i * C;
        const float nrm = moco_row_norm(fr, C, lane);
        for (int c = lane; c < C; c += 64) s_q[i * C + c] = fr[c] / nrm;
    }
    if (t < n) { s_m[t] = -INFINITY; s_s[t] = 0.f; }

    const int j_begin = blockIdx.x * p.slab_rows;
    const int j_end = j_begin + p.slab_rows < p.K ? j_begin + p.slab_rows : p.K;
    f32x4 pf[PF];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int e = t + SF_THREADS * k, row = e / C4, c4 = e - row * C4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + row < j_end) v = *reinterpret_cast<const f32x4*>(p.queue + (int64_t)(j0 + row) * C + 4 * c4);
            pf[k] = v;
        }
    };
    fetch(j_begin);

    // A update: thread (cg, ig) owns columns 4 cg .. 4 cg + 3 of query rows ig, ig + IG, ...
    const int cg = t % C4, ig = t / C4;
    const int rp = ig < IG && ig < n ? (n - ig + IG - 1) / IG : 0;
    f32x4 acc[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j0 = j_begin; j0 < j_end; j0 += SF_MOCO_CHUNK) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int e = t + SF_THREADS * k, row = e / C4, c4 = e - row * C4;
            *reinterpret_cast<f32x4*>(&s_t[row * LDT + 4 * c4]) = pf[k];
        }
        __syncthreads();
        if (j0 + SF_MOCO_CHUNK < j_end) fetch(j0 + SF_MOCO_CHUNK);

        // logits of the chunk: lane = queue row, a wave takes four query rows at a time
        const int j = j0 + lane;
        const bool jv = j < j_end;
        for (int ib = 4 * w; ib < n; ib += 4 * (SF_THREADS / 64)) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            int ir[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) ir[b] = ib + b < n ? ib + b : n - 1;
            for (int c4 = 0; c4 < C4; ++c4) {
                const f32x4 tv = *reinterpret_cast<const f32x4*>(&s_t[lane * LDT + 4 * c4]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>(&s_q[ir[b] * C + 4 * c4]);
                    d[b] += qv[0] * tv[0];
                    d[b] += qv[1] * tv[1];
                    d[b] += qv[2] * tv[2];
                    d[b] += qv[3] * tv[3];
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = ib + b;
                const bool iv = i < n;                  // wave-uniform
                const float l = jv ? d[b] * p.invT : -INFINITY;
                if (iv && jv)
                    for (int v = 0; v < p.V; ++v) p.logits[((int64_t)v * n + i) * ldl + 1 + j] = l;
                const float mold = s_m[ir[b]];
                const float mnew = fmaxf(mold, moco_wave_max(l));       // finite: the chunk holds at least one queue row
                const float ex = jv ? expf(l - mnew) : 0.f;
                if (iv) s_e[i * LDE + lane] = ex;
                const float se = moco_wave_sum(ex);
                if (iv && lane == 0) {
                    const float al = expf(mold - mnew);                 // 0 on the first chunk (mold = -inf)
                    s_s[i] = s_s[i] * al + se;
                    s_m[i] = mnew;
                    s_al[i] = al;
                }
            }
        }
        __syncthreads();

#pragma unroll
        for (int r = 0; r < RP; ++r)
            if (r < rp) acc[r] *= s_al[ig + IG * r];
        for (int j4 = 0; j4 < SF_MOCO_CHUNK / 4; ++j4) {
            f32x4 tv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) tv[u] = *reinterpret_cast<const f32x4*>(&s_t[(4 * j4 + u) * LDT + 4 * cg]);
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                if (r < rp) {
                    const f32x4 ev = *reinterpret_cast<const f32x4*>(&s_e[(ig + IG * r) * LDE + 4 * j4]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[r] += ev[u] * tv[u];
                }
            }
        }
        __syncthreads();
    }

    const int64_t base = (int64_t)blockIdx.x * n;
    if (t < n) {
        p.ws_ms[(base + t) * 2] = s_m[t];
        p.ws_ms[(base + t) * 2 + 1] = s_s[t];
    }
#pragma unroll
    for (int r = 0; r < RP; ++r)
        if (r < rp) *reinterpret_cast<f32x4*>(p.ws_a + (base + ig + IG * r) * C + 4 * cg) = acc[r];
}

// M and S of query row i over all slabs, by ONE wave: lane l loads slabs l, l + 64, ... (at most SF_MOCO_SLABS / 64 each), the
// maximum is a 6-step fold (exact in any order), every slab's weight w_s = exp(M_s - M) and term S_s w_s go to the wave's LDS
// rows, and every lane then adds the terms in slab order.  Every caller runs this routine: the same bits everywhere.
__device__ __forceinline__ void moco_row_ms(const MocoNceParams& p, int i, int lane, float* s_w, float* s_ts, float& M, float& S) {
    constexpr int PER = SF_MOCO_SLABS / 64;
    float mk[PER], sk[PER];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = lane + 64 * k;
        mk[k] = -INFINITY;
        sk[k] = 0.f;
        if (s < p.nslab) {
            const float* ms = p.ws_ms + ((int64_t)s * p.n + i) * 2;
            mk[k] = ms[0];
            sk[k] = ms[1];
        }
        mx = fmaxf(mx, mk[k]);
    }
    M = moco_wave_max(mx);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = lane + 64 * k;
        if (s < p.nslab) {
            const float wgt = expf(mk[k] - M);
            s_w[s] = wgt;
            s_ts[s] = sk[k] * wgt;
        }
    }
    SF_WAVE_LDS_SYNC();
    float acc = 0.f;
    for (int s = 0; s < p.nslab; ++s) acc += s_ts[s];                  // slab order
    S = acc;
}

// One wave: norm of f_i, M, S, and per view the positive logit, lse, p0 = exp(l_pos - lse), ca = exp(M - lse).
// out (LDS, written by lane 0): [0] |f_i|  [1] M  [2] S  [4 + 4 v ..] l_pos, lse, p0, ca;  s_w keeps the slab weights
__device__ __forceinline__ void moco_row_terms(const MocoNceParams& p, int i, int lane, float* s_w, float* s_ts, float* out) {
    const float* fr = p.f + (int64_t)i * p.C;
    const float nrm = moco_row_norm(fr, p.C, lane);
    float M, S;
    moco_row_ms(p, i, lane, s_w, s_ts, M, S);
    if (lane == 0) { out[0] = nrm; out[1] = M; out[2] = S; }
    for (int v = 0; v < p.V; ++v) {
        const float* kr = p.key + ((int64_t)v * p.n + i) * p.C;
        float d = 0.f;
        for (int c = lane; c < p.C; c += 64) d += (fr[c] / nrm) * kr[c];
        const float lpos = moco_wave_sum(d) * p.invT;
        const float mp = fmaxf(M, lpos);
        const float lse = mp + logf(expf(lpos - mp) + S * expf(M - mp));
        if (lane == 0) {
            out[4 + 4 * v] = lpos;
            out[5 + 4 * v] = lse;
            out[6 + 4 * v] = expf(lpos - lse);
            out[7 + 4 * v] = expf(M - lse);
        }
    }
    SF_WAVE_LDS_SYNC();             // the next row of this wave overwrites s_w / s_ts
}

// grid = n + 1: workgroup i < n finishes query row i (column 0 of its V logits rows, df_i); workgroup n sums the loss
__global__ __launch_bounds__(SF_THREADS) void sf_moco_nce_finalize_kernel(MocoNceParams p) {
    __shared__ float s_row[4][4 + 4 * SF_MOCO_VMAX];
    __shared__ float s_w[4][SF_MOCO_SLABS], s_ts[4][SF_MOCO_SLABS];
    __shared__ float s_term[SF_MOCO_VMAX * (SF_MOCO_QMAX / 64)];
    __shared__ float s_red[SF_THREADS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = p.n, C = p.C;
    const int R = p.V * n;
    if ((int)blockIdx.x == n) {
        for (int i = w; i < n; i += SF_THREADS / 64) {
            moco_row_terms(p, i, lane, s_w[w], s_ts[w], s_row[w]);
            if (lane == 0)          // lane 0 wrote the row's terms and lane 0 reads them
                for (int v = 0; v < p.V; ++v) s_term[v * n + i] = s_row[w][5 + 4 * v] - s_row[w][4 + 4 * v];
        }
        __syncthreads();
        if (t == 0) {
            float sum = 0.f;
            for (int r = 0; r < R; ++r) sum += s_term[r];           // row order
            p.loss[0] = sum / (float)R;
        }
        return;
    }
    const int i = blockIdx.x;
    if (w == 0) moco_row_terms(p, i, lane, s_w[0], s_ts[0], s_row[0]);
    __syncthreads();
    const float nrm = s_row[0][0];
    // A_i[c] = sum_s w_s A_s[c]: SF_THREADS / C groups of threads take contiguous runs of slabs in slab order (independent
    // loads, unrolled), the groups' partial sums are then added in group order
    const int G = SF_THREADS / C, g = t / C, c = t - g * C;
    const int per = (p.nslab + G - 1) / G;
    if (g < G) {
        const int s0 = g * per, s1 = s0 + per < p.nslab ? s0 + per : p.nslab;
        float a = 0.f;
#pragma unroll 8
        for (int s = s0; s < s1; ++s) a += p.ws_a[((int64_t)s * n + i) * C + c] * s_w[0][s];
        s_red[t] = a;
    }
    __syncthreads();
    float qc = 0.f, dq = 0.f;
    if (t < C) {
        float a = 0.f;
        for (int k = 0; k < G; ++k) a += s_red[k * C + t];
        qc = p.f[(int64_t)i * C + t] / nrm;
        for (int v = 0; v < p.V; ++v)
            dq += (s_row[0][6 + 4 * v] - 1.f) * p.key[((int64_t)v * n + i) * C + t] + s_row[0][7 + 4 * v] * a;
        dq *= p.invT / (float)R;
    }
    if (t < p.V) p.logits[((int64_t)t * n + i) * ((int64_t)p.K + 1)] = s_row[0][4 + 4 * t];
    __syncthreads();                // s_red is reused
    s_red[t] = qc * dq;
    __syncthreads();
    for (int h = SF_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) s_red[t] += s_red[t + h];
        __syncthreads();
    }
    if (t < C) p.df[(int64_t)i * C + t] = (dq - qc * s_red[0]) / nrm;
}

// ------------------------------------------------------------------------------------------------
// _dequeue_and_enqueue: `views` blocks of `rows` keys are written at the pointer, one after the other, the pointer wrapping to
// 0 when it reaches K.  ONE workgroup: every thread reads the pointer, a barrier, the copy, then thread 0 stores the new
// pointer -- a grid of several workgroups could not order "all have read it" before "it is updated" without a second launch.
// A pointer from which one of the writes would leave [0, K) makes the call a no-op that raises the error word.
struct EnqueueParams {
    const float* keys;      // [views][rows][C]
    float* queue;           // [K][C]
    int64_t* ptr;
    int32_t* err;
    int K, C, rows, views;
    int vec;                // 16-byte accesses are aligned
};
__global__ __launch_bounds__(SF_THREADS) void sf_queue_enqueue_kernel(EnqueueParams p) {
    const int64_t ptr0 = p.ptr[0];
    __syncthreads();
    bool ok = true;
    int64_t q = ptr0;
    for (int v = 0; v < p.views; ++v) {
        if (q < 0 || q + p.rows > p.K) { ok = false; break; }
        q += p.rows;
        if (q == p.K) q = 0;
    }
    if (!ok) {
        if (threadIdx.x == 0) p.err[0] = 1;
        return;
    }
    const int64_t per = (int64_t)p.rows * p.C;
    q = ptr0;
    for (int v = 0; v < p.views; ++v) {
        const float* src = p.keys + v * per;
        float* dst = p.queue + q * p.C;
        if (p.vec) {
            for (int64_t e = threadIdx.x; e < per / 4; e += SF_THREADS)
                *reinterpret_cast<f32x4*>(dst + 4 * e) = *reinterpret_cast<const f32x4*>(src + 4 * e);
        } else {
            for (int64_t e = threadIdx.x; e < per; e += SF_THREADS) dst[e] = src[e];
        }
        q += p.rows;
        if (q == p.K) q = 0;
    }
    if (threadIdx.x == 0) p.ptr[0] = q;
}

// ------------------------------------------------------------------------------------------------
// `dist[name].data * (1.0 - m) + p.data * m`: three separately rounded fp32 operations (contraction off, as mix2() of
// sf_mixup.h); mm = {fp32(m), fp32(1.0 - m)} with the difference taken in double by the host.
__device__ __forceinline__ float ema2(float pv, float hv, float m, float omm) {
#pragma clang fp contract(off)
    const float a = pv * omm;
    const float b = hv * m;
    return a + b;
}
struct EmaParams {
    const float* p;
    float* hist;
    const float* mm;
    int64_t n;
    int vec;
};
__global__ __launch_bounds__(SF_THREADS) void sf_ema_update_kernel(EmaParams p) {
    const float m = p.mm[0], omm = p.mm[1];
    const int64_t stride = (int64_t)gridDim.x * SF_THREADS, first = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
    if (p.vec) {
        const int64_t n4 = p.n >> 2;
        for (int64_t i = first; i < n4; i += stride) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p.p + 4 * i);
            const f32x4 h = *reinterpret_cast<const f32x4*>(p.hist + 4 * i);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ema2(a[e], h[e], m, omm);
            *reinterpret_cast<f32x4*>(p.hist + 4 * i) = o;
        }
        if (blockIdx.x == 0)
            for (int64_t i = 4 * n4 + threadIdx.x; i < p.n; i += SF_THREADS) p.hist[i] = ema2(p.p[i], p.hist[i], m, omm);
    } else {
        for (int64_t i = first; i < p.n; i += stride) p.hist[i] = ema2(p.p[i], p.hist[i], m, omm);
    }
}
