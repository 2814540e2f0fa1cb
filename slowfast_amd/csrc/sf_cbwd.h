// Block-final BatchNorm backward fused into both gradients of the block's last (1x1x1) convolution (gfx950).
//
//   dy_c = (f16)(k1 * g + k2 + k3 * yc),  g = dz under the block output's 1-bit ReLU mask     (sf_bn_bwd_apply_kernel, sf_bn.h)
//   d_in[m][ci]  = sum_co dy_c[m][co] * Wd[ci][co]                                             (sf_conv_dgrad_bn)
//   dW[co][ci]  += sum_m  dy_c[m][co] * act_b[m][ci]                                           (sf_conv_wgrad)
//
// (BottleneckTransform c + c_bn, slowfast/models/resnet_helper.py:361-369, and the tail of ResBlock.forward :512-521.)  dy_c is as
// wide as the block output and has exactly these two readers, both with a tiny second operand: the three launches move it through
// HBM three times (one write, two reads) on top of the two reads that produce it.  Here a workgroup forms dy_c for a tile of R rows
// in LDS and feeds both products from that tile; dy_c never reaches global memory.
//
//   * a workgroup walks many row tiles with its weight-gradient accumulators in registers; no atomics, no hand-off between
//     workgroups, no grid barrier.  WHICH rows it walks is what sf_conv_wgrad's plan gives one split of the same layer (sf_api.hip:
//     a contiguous run of 32-row chunks, or -- the thin plan, Co <= 32 -- the 128-row stages b, b + G, ... with the four waves a
//     quarter of each stage): every 32-row MFMA step then lands on the accumulator it lands on in the three-launch path, in the
//     same order, the slabs meet in the same sf_wgrad_reduce_kernel launch, and dw is bit for bit what that path computes.  A
//     128-row table tile that straddles two runs is formed by both workgroups: each takes the weight-gradient steps of its own rows
//     (the act_b rows of the other run are copied as zeros), the one that holds the tile's first row also takes its data gradient;
//   * stage 1: the RowTile thread map (a thread keeps its 8-channel group; COP / 8 threads across a row): 16-byte loads of dz and
//     yc + the mask byte, the expression of sf_bn_bwd_apply_kernel, the rounded value stored to the LDS tile [R][COP + 8] (the pad
//     keeps the 16-byte fragment reads of the data gradient conflict-free).  The loads of the NEXT tile are issued right after the
//     tile is written and stay in flight under both MFMA phases;
//   * act_b tile: direct global -> LDS copies (lane-linear [R][CIP]), issued for the next tile as soon as the weight-gradient phase
//     has read the current one;
//   * Wd ([CIP][COP + 8]) and the three coefficient rows are loaded once per workgroup;
//   * weight gradient: dW tile = Dy^T . Act from transposed LDS fragment reads (ds_read_b64_tr_b16), the waves split the output
//     channels (COP = 32: the rows, and their four partial tiles are summed through LDS at the end, as sf_wgrad2t_kernel does); the
//     accumulators live in registers across all tiles of the workgroup and leave ONE fp32 slab per workgroup;
//   * data gradient: the waves split the rows; the fp16-rounded tile is staged through LDS (over the dead Dy tile), stored with
//     16-byte rows, and the BatchNorm-backward sums of the INNER BatchNorm are taken from the stored values (bnb_accumulate /
//     bnb_reduce_store of sf_igemm.h): one table row per 128 rows, a thread's sums running over the 128 / R tiles in row order --
//     the tiles and the per-thread order of the 128-row data-gradient epilogue, so the table has that epilogue's bits.
// CIP / COP are the channel counts rounded up to {16, 32, 64, 128} / {32, 64, 128, 256}; the real counts are runtime values (columns
// beyond them are zeros in LDS and never stored).
//
// The projection shortcut of a stage's first block (branch1 + branch1_bn, resnet_helper.py:485-499) has the same backward with the
// block INPUT in the place of act_b and no inner BatchNorm (sf_conv_proj_bwd): Ci up to 128 (CIP 128: the Wd tile alone is up to
// 66 KB, one workgroup per CU at COP 256), and a spatial stride of 2 as a row map -- output row (n, t, ho, wo) reads the act row
// (n, t, 2 ho, 2 wo), its d_in goes to that row, and the owner of the output row stores the other three input rows of the 2 x 2
// cell as zeros: d_in is written completely, as the residue-class launches of the strided data gradient write it.
#pragma once
#include "sf_bn.h"
#include "sf_common.h"
#include "sf_igemm.h"

struct CbwdParams {
    int M, Ci, Co;
    const f16* dz; int lddz;
    const uint8_t* bits;            // [M][Co / 8]
    const f16* yc; int ldyc;
    const float* coef;              // [3][Co]
    const f16* act; int ldact;      // [M][Ci]
    const f16* wd; int ldw;         // [Ci][ldw], columns co
    const f16* bnb_y; int bnb_ld;   // optional fused reduction (bnb_part == nullptr: off)
    const float* bnb_scale; const float* bnb_shift;
    float* bnb_part;                // [ntiles][2][Ci]
    f16* dx; int lddx;
    float* ws;                      // [gridDim.x][COP][CIP] fp32
    int rps;                        // > 0: workgroup b owns the rows [b * rps, (b + 1) * rps) (a multiple of 32); 0: 128-row tiles b, b + G, ...
    int tiles128;                   // ceil(M / 128)
    int str2;                       // spatial stride 2 (Hi = 2 Ho, Wi = 2 Wo): M counts OUTPUT rows, act / dx have 4 M rows
    FastDiv fdWo;                   // (str2) output row m = q * Wo + wo  ->  input row 4 Wo q + 2 wo
};

template <int CIP, int COP>
struct CbwdCfg {
    static constexpr int R = COP >= 128 ? 64 : 128;                         // rows per tile; NSUB tiles make one 128-row table tile
    static constexpr int NSUB = 128 / R;
    static constexpr int NJ = CIP / 16, KS = COP / 32, TI = R / 64;
    static constexpr int WAVES_M = COP == 32 ? 4 : 1, WAVES_C = 4 / WAVES_M;   // COP = 32: the waves split the rows (sf_wgrad2t_kernel's order)
    static constexpr int TC = COP / 16 / WAVES_C;
    static constexpr int KSM = R / WAVES_M / 32;                            // 32-row steps of one wave's weight-gradient rows
    static constexpr int LDY = COP + 8;
    static constexpr int CGO = COP / 8, RPP = SF_THREADS / CGO, NCH = R / RPP;   // stage 1: chunks per row, rows per pass, chunks per thread
    static constexpr int ACH = CIP / 8, NACT = R * ACH / 64;                // act tile: chunks per row, copy instructions
    static constexpr int NEPI = (R * ACH + SF_THREADS - 1) / SF_THREADS;    // d_in chunks per thread
    static constexpr int DY_ELEMS = R * LDY, ACT_ELEMS = R * CIP, WD_ELEMS = CIP * LDY;
    static constexpr int RED_ELEMS = 4 * ACH * 24 * 2;                      // bnb_reduce_store scratch, in f16 units
    static constexpr int UNION_ELEMS = DY_ELEMS > ACT_ELEMS + RED_ELEMS ? DY_ELEMS : ACT_ELEMS + RED_ELEMS;
    static constexpr int LDS_ELEMS = UNION_ELEMS + ACT_ELEMS + WD_ELEMS + 3 * COP * 2 + 2 * CIP * 2;
    static_assert(WAVES_M == 1 || LDS_ELEMS * 2 >= 4 * (COP / 16) * NJ * 256 * 4, "the cross-wave sum reuses the tile buffers");
    static constexpr int LDS_BYTES = LDS_ELEMS * 2;
    // registers a thread holds across the MFMA phases: accumulators + the next tile's operands
    static constexpr int HELD = 4 * NJ * (TI + TC) + 9 * NCH + 4 * NEPI;
    static constexpr int OCC_REGS = HELD <= 72 ? 3 : 2;
    static constexpr int OCC_LDS = 160 * 1024 / LDS_BYTES;
    static constexpr int OCC = OCC_LDS < OCC_REGS ? OCC_LDS : OCC_REGS;     // waves per SIMD = workgroups per CU
    static_assert(R % 64 == 0 && R % RPP == 0 && NACT >= 1 && (R * ACH) % 64 == 0, "tile shape");
    static_assert(SF_THREADS % ACH == 0 && 64 % ACH == 0, "a thread keeps one d_in column group");
};

template <int CIP, int COP>
__global__ __launch_bounds__(SF_THREADS, (CbwdCfg<CIP, COP>::OCC)) void sf_cbwd_kernel(CbwdParams p) {
    using K = CbwdCfg<CIP, COP>;
    constexpr int R = K::R, LDY = K::LDY, NJ = K::NJ, TI = K::TI, TC = K::TC;
    __shared__ __attribute__((aligned(16))) f16 smem[K::LDS_ELEMS];
    f16* const DyL = smem;                                      // [R][LDY]; later the staged d_in tile [R][CIP] + the reduction scratch
    f16* const StL = smem;
    float* const red = reinterpret_cast<float*>(smem + K::ACT_ELEMS);
    f16* const ActL = smem + K::UNION_ELEMS;                    // [R][CIP], lane-linear
    f16* const WdL = ActL + K::ACT_ELEMS;                       // [CIP][LDY]
    float* const coefL = reinterpret_cast<float*>(WdL + K::WD_ELEMS);   // [3][COP]
    float* const bnL = coefL + 3 * COP;                         // [2][CIP]: scale, shift of the inner BatchNorm

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 15, g4 = lane >> 4;
    const int G = (int)gridDim.x;
    const f16* const zline = reinterpret_cast<const f16*>(sf_zero_line);
    const bool bnb = p.bnb_part != nullptr;

    // ---- once per workgroup: Wd and the coefficients
    for (int q = tid; q < CIP * K::CGO; q += SF_THREADS) {
        const int ci = q / K::CGO, cg = q % K::CGO;
        f16x8 v = zero8();
        if (ci < p.Ci && cg * 8 < p.Co) v = ld16(p.wd + (int64_t)ci * p.ldw + cg * 8);
        st16(WdL + ci * LDY + cg * 8, v);
    }
    for (int q = tid; q < 3 * COP; q += SF_THREADS) {
        const int k = q / COP, c = q % COP;
        coefL[q] = c < p.Co ? p.coef[k * p.Co + c] : 0.f;
    }
    for (int q = tid; q < 2 * CIP; q += SF_THREADS) {
        const int k = q / CIP, c = q % CIP;
        bnL[q] = (bnb && c < p.Ci) ? (k ? p.bnb_shift[c] : p.bnb_scale[c]) : (k ? 0.f : 1.f);
    }

    // ---- stage-1 thread map: column group scg of rows srow + u * RPP
    const int scg = tid % K::CGO, srow = tid / K::CGO;
    const bool scol_ok = scg * 8 < p.Co;
    const int scgc = scol_ok ? scg : 0;                         // clamped: every load below is unconditional (no branch per load)
    // ---- d_in thread map: column group ecg of rows (tid + e * 256) / ACH
    const int ecg = tid % K::ACH;
    const bool ecol_ok = ecg * 8 < p.Ci;
    const int ecgc = ecol_ok ? ecg : 0;

    // ---- the tiles this workgroup walks
    int r0 = 0, r1 = p.M, T0 = (int)blockIdx.x, Tstep = G, nwalk = 0;
    if (p.rps > 0) {
        r0 = (int)blockIdx.x * p.rps;
        r1 = r0 + p.rps < p.M ? r0 + p.rps : p.M;
        T0 = r0 >> 7;
        Tstep = 1;
        if (r1 > r0) nwalk = (((r1 + 127) >> 7) - T0) * K::NSUB;
    } else if (T0 < p.tiles128) nwalk = ((p.tiles128 - 1 - T0) / G + 1) * K::NSUB;
    auto tile_m0 = [&](int q) { return (T0 + (q / K::NSUB) * Tstep) * 128 + (q % K::NSUB) * R; };
    // the act / d_in row of output row m
    const int Wi = 2 * (int)p.fdWo.d;
    auto in_row = [&](int m) -> int64_t {
        if (!p.str2) return m;
        uint32_t qr, wo;
        fd_divmod((uint32_t)m, p.fdWo, qr, wo);
        return (int64_t)qr * (2 * Wi) + 2 * wo;
    };

    f16x8 dzr[K::NCH], ycr[K::NCH], ybr[K::NEPI];
    uint32_t mbr[K::NCH];
    auto load_regs = [&](int m0) {
#pragma unroll
        for (int u = 0; u < K::NCH; ++u) {
            int m = m0 + srow + u * K::RPP;
            if (m > p.M - 1) m = p.M - 1;
            dzr[u] = ld16(p.dz + (int64_t)m * p.lddz + scgc * 8);
            ycr[u] = ld16(p.yc + (int64_t)m * p.ldyc + scgc * 8);
            mbr[u] = p.bits[(int64_t)m * (p.Co >> 3) + scgc];
        }
    };
    // the inner BatchNorm's y rows of the CURRENT tile: issued before the data-gradient MFMAs, consumed by the store loop
    auto load_yb = [&](int m0) {
#pragma unroll
        for (int e = 0; e < K::NEPI; ++e) {
            int m = m0 + (tid + e * SF_THREADS) / K::ACH;
            if (m > p.M - 1) m = p.M - 1;
            ybr[e] = ld16(p.bnb_y + (int64_t)m * p.bnb_ld + ecgc * 8);
        }
    };
    auto issue_act = [&](int m0) {
#pragma unroll
        for (int j = 0; j < (K::NACT + 3) / 4; ++j) {
            const int q = wave + 4 * j;                         // copy instruction: 64 chunks = 64 / ACH rows
            if (q < K::NACT) {
                const int c = q * 64 + lane;
                const int m = m0 + c / K::ACH, cc = c % K::ACH;
                const f16* g = (m >= r0 && m < r1 && cc * 8 < p.Ci) ? p.act + in_row(m) * p.ldact + cc * 8 : zline;
                SF_GLOBAL_LOAD_LDS16_ASM(g, ActL + q * 512);
            }
        }
    };


    f32x4 wacc[TC][NJ];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) wacc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wc = wave % K::WAVES_C, wm = wave / K::WAVES_C;
    const int cobase = wc * TC * 16, mbase = wm * (R / K::WAVES_M);
    const int rowbase = wave * (R / 4);

    float bsg[8], bsgy[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { bsg[e] = 0.f; bsgy[e] = 0.f; }
    const int nq = nwalk;
    if (nq > 0) { load_regs(tile_m0(0)); issue_act(tile_m0(0)); }
    for (int q = 0; q < nq; ++q) {
        const int m0 = tile_m0(q);
        const int T = T0 + (q / K::NSUB) * Tstep;               // the 128-row table tile this tile belongs to
        const bool owner = T * 128 >= r0 && T * 128 < r1;       // d_in and the table row of T come from the workgroup that holds its first row
        const bool more = q + 1 < nq;
        SF_WAIT_VMEM();                                         // this wave's operands of the tile (registers and act copies) have landed
        __syncthreads();                                        // the previous tile's staged d_in / reduction scratch is dead (first tile: Wd, coef)
        // ---- stage 1: dy_c tile
        {
            float k1[8], k2[8], k3[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { k1[e] = coefL[scg * 8 + e]; k2[e] = coefL[COP + scg * 8 + e]; k3[e] = coefL[2 * COP + scg * 8 + e]; }
#pragma unroll
            for (int u = 0; u < K::NCH; ++u) {
                const int row = srow + u * K::RPP;
                const uint32_t b = mbr[u];
                const f16x8 yv = ycr[u];
                float g[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) g[e] = (float)dzr[u][e];
#pragma unroll
                for (int e = 0; e < 8; ++e) g[e] = ((b >> e) & 1u) ? g[e] : 0.f;
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (f16)(k1[e] * g[e] + k2[e] + k3[e] * (float)yv[e]);
                if (!(scol_ok && m0 + row < p.M)) o = zero8();
                st16(DyL + row * LDY + scg * 8, o);
            }
        }
        __syncthreads();                                        // Dy and Act tiles complete
        if (more) load_regs(tile_m0(q + 1));                    // in flight under both MFMA phases
        // ---- weight gradient: wacc += Dy^T . Act over this wave's rows
#pragma unroll
        for (int ks = 0; ks < K::KSM; ++ks) {
            f16x8 af[TC], bf[NJ];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int m = mbase + ks * 32 + 8 * g4 + 4 * h + (pl >> 2);
#pragma unroll
                for (int i = 0; i < TC; ++i) {
                    const f16x4 v = as_f16x4(SF_LDS_TR16(DyL + m * LDY + cobase + i * 16 + 4 * (pl & 3)));
                    af[i][4 * h + 0] = v[0]; af[i][4 * h + 1] = v[1]; af[i][4 * h + 2] = v[2]; af[i][4 * h + 3] = v[3];
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const f16x4 v = as_f16x4(SF_LDS_TR16(ActL + m * CIP + j * 16 + 4 * (pl & 3)));
                    bf[j][4 * h + 0] = v[0]; bf[j][4 * h + 1] = v[1]; bf[j][4 * h + 2] = v[2]; bf[j][4 * h + 3] = v[3];
                }
            }
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) wacc[i][j] = SF_MFMA16(af[i], bf[j], wacc[i][j]);
        }
        SF_BARRIER_KEEP_VMEM();                                 // every wave has read the Act tile
        if (more) issue_act(tile_m0(q + 1));
        if (!owner) continue;                                   // (workgroup-uniform) this tile only fed the weight gradient
        if (bnb) load_yb(m0);
        // ---- data gradient: rows rowbase .. rowbase + R / 4 of the tile
        f32x4 dacc[TI][NJ];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) dacc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < K::KS; ++ks) {
            f16x8 bf[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bf[j] = ld16(WdL + (j * 16 + pl) * LDY + ks * 32 + 8 * g4);
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const f16x8 af = ld16(DyL + (rowbase + i * 16 + pl) * LDY + ks * 32 + 8 * g4);
#pragma unroll
                for (int j = 0; j < NJ; ++j) dacc[i][j] = SF_MFMA16(af, bf[j], dacc[i][j]);
            }
        }
        SF_BARRIER_KEEP_VMEM();                                 // every wave has read the Dy tile: stage d_in over it
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) StL[(rowbase + i * 16 + 4 * g4 + r) * CIP + j * 16 + pl] = (f16)dacc[i][j][r];
        SF_BARRIER_KEEP_VMEM();
        float bsc[8], bsh[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { bsc[e] = bnL[ecg * 8 + e]; bsh[e] = bnL[CIP + ecg * 8 + e]; }
#pragma unroll
        for (int e = 0; e < K::NEPI; ++e) {
            const int idx = tid + e * SF_THREADS;
            const int row = idx / K::ACH, m = m0 + row;
            if (idx < R * K::ACH && m < p.M && ecol_ok) {
                const f16x8 v = ld16(StL + row * CIP + ecg * 8);
                f16* const o = p.dx + in_row(m) * p.lddx + ecg * 8;
                st16(o, v);
                if (p.str2) {                                   // the three unsampled rows of the 2 x 2 cell
                    st16(o + p.lddx, zero8());
                    st16(o + (int64_t)Wi * p.lddx, zero8());
                    st16(o + (int64_t)(Wi + 1) * p.lddx, zero8());
                }
                if (bnb) bnb_accumulate(v, ybr[e], bsc, bsh, bsg, bsgy, false, 0u);
            }
        }
        // a thread's sums run over the NSUB tiles of a table tile in row order (the order of the 128-row data-gradient epilogue)
        if (bnb && q % K::NSUB == K::NSUB - 1) {
            bnb_reduce_store<4, K::ACH>(bsg, bsgy, red, p.bnb_part + (int64_t)T * 2 * p.Ci, 0, p.Ci);
#pragma unroll
            for (int e = 0; e < 8; ++e) { bsg[e] = 0.f; bsgy[e] = 0.f; }
        }
    }

    // ---- one fp32 slab per workgroup (zeros when it had no rows)
    float* slab = p.ws + (int64_t)blockIdx.x * (COP * CIP);
    if constexpr (K::WAVES_M == 4) {
        // the four waves' partial tiles, summed through LDS as sf_wgrad2t_kernel sums them
        __syncthreads();
        float* rd = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) rd[(((wave * TC + i) * NJ + j) * 4 + r) * 64 + lane] = wacc[i][j][r];
        __syncthreads();
        constexpr int TE = TC * NJ * 256;
        for (int e = tid; e < TE; e += SF_THREADS) {
            const float v = (rd[e] + rd[TE + e]) + (rd[2 * TE + e] + rd[3 * TE + e]);
            const int ln = e & 63, r = (e >> 6) & 3, tt = e >> 8;
            const int i = tt / NJ, j = tt - i * NJ;
            slab[(i * 16 + 4 * (ln >> 4) + r) * CIP + j * 16 + (ln & 15)] = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) slab[(cobase + i * 16 + 4 * g4 + r) * CIP + j * 16 + pl] = wacc[i][j][r];
    }
}
