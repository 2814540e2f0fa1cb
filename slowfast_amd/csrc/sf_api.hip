// C ABI of libsfamd.so (declared in include/sfamd.h): argument validation, tile selection, launches.
#include "../../include/sfamd.h"
#include "sf_bn.h"
#include "sf_common.h"
#include "sf_igemm.h"
#include "sf_igemm2.h"
#include "sf_gconv.h"
#include "sf_wgrad2.h"
#include "sf_cbwd.h"
#include "sf_pool.h"
#include "sf_dwconv.h"
#include "sf_dwsweep.h"
#include "sf_dwtemporal.h"
#include "sf_tokens.h"
#include "sf_x3d.h"
#include "sf_stem.h"
#include "sf_attn.h"
#include "sf_roi.h"
#include "sf_optim.h"
#include "sf_mixup.h"
#include "sf_erase.h"
#include "sf_pack.h"
#include "sf_sample.h"
#include "sf_color.h"
#include "sf_randaug.h"
#include "sf_sslcolor.h"
#include "sf_hog.h"
#include "sf_pixel.h"
#include "sf_moco.h"
#include "sf_byol.h"
#include "sf_simclr.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}
#define REQUIRE(cond, ...) \
    do { if (!(cond)) return fail(__VA_ARGS__); } while (0)

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int roundup(int a, int b) { return (a + b - 1) / b * b; }

// Environment switches, two classes (47 getenv sites, many per launch, each an untested product configuration):
//   test_hook(name, default)  dispatch thresholds the TEST SUITE lowers so that small shapes reach a kernel (SF_IGEMM2_MINK ...),
//                             kernel selectors its parity cases flip (SF_DW_SWEEP ...) and SF_TRACE: read in every build;
//   tune_knob(name, default)  A/B knobs whose optimum was measured (block targets, occupancy caps, variant selectors; the
//                             evidence is under profiles/): COMPILE-TIME constants in the product build, overridable only in
//                             -DSF_DIAG builds (libsfamd_diag.so, tools/ sweeps).
static inline int test_hook(const char* name, int def) { const char* e = getenv(name); return e ? atoi(e) : def; }
#ifdef SF_DIAG
static inline int tune_knob(const char* name, int def) { const char* e = getenv(name); return e ? atoi(e) : def; }
#else
#define tune_knob(name, def) (def)
#endif

extern "C" int sf_abi_version(void) { return SF_ABI_VERSION; }
// "gfx950" for the hipcc build; the host functional simulator used by the CPU tests reports itself.
extern "C" const char* sf_backend(void) {
#ifdef SF_HOSTSIM
    return "hostsim";
#else
    return "gfx950";
#endif
}
extern "C" int sf_act_dtype(void) { return SF_ACT_DTYPE_ID; }
extern "C" const char* sf_last_error(void) { return g_err; }
// hash of the sources this binary was compiled from (slowfast_amd/build_ext.py passes it; lib.SfLibrary compares it with the
// sources shipped beside the binary and refuses a stale one)
#ifndef SF_BUILD_ID
#define SF_BUILD_ID "unversioned"
#endif
extern "C" const char* sf_build_id(void) {
    static const char tagged[] = "sfamd-build-id:" SF_BUILD_ID;
    return tagged + 15;
}

static int check_desc(const sf_conv_desc* d) {
    REQUIRE(d != nullptr, "conv: null descriptor");
    REQUIRE(d->N > 0 && d->Ci > 0 && d->Co > 0, "conv: empty tensor");
    REQUIRE(d->Ci % 8 == 0 && d->Co % 8 == 0, "conv: channel counts must be multiples of 8 (Ci=%d Co=%d)", d->Ci, d->Co);
    REQUIRE(d->ldx >= d->Ci && d->ldx % 8 == 0 && d->ldy >= d->Co && d->ldy % 8 == 0, "conv: bad row pitch");
    REQUIRE(d->Cw > 0 && d->Cw <= d->Ci, "conv: Cw must be in (0, Ci]");
    REQUIRE(d->Cow >= 0 && d->Cow <= d->Co, "conv: Cow must be in [0, Co]");
    REQUIRE(d->sT > 0 && d->sH > 0 && d->sW > 0 && d->dT > 0 && d->dH > 0 && d->dW > 0, "conv: stride/dilation");
    int To = (d->Ti + 2 * d->pT - d->dT * (d->kT - 1) - 1) / d->sT + 1;
    int Ho = (d->Hi + 2 * d->pH - d->dH * (d->kH - 1) - 1) / d->sH + 1;
    int Wo = (d->Wi + 2 * d->pW - d->dW * (d->kW - 1) - 1) / d->sW + 1;
    // fewer outputs than the formula gives = trailing output positions dropped (asymmetric end padding; used by
    // the W-pair-folded stem convolutions); more would read outside the padded input
    REQUIRE(d->To >= 1 && d->Ho >= 1 && d->Wo >= 1 && d->To <= To && d->Ho <= Ho && d->Wo <= Wo,
            "conv: output dims (%d,%d,%d) exceed the geometry's (%d,%d,%d)", d->To, d->Ho, d->Wo, To, Ho, Wo);
    int64_t Mo = (int64_t)d->N * d->To * d->Ho * d->Wo, Mi = (int64_t)d->N * d->Ti * d->Hi * d->Wi;
    REQUIRE(Mo < (1ll << 31) && Mi < (1ll << 31), "conv: more than 2^31 positions");
    return 0;
}

static void fill_gather_common(GatherSide& g, const sf_conv_desc* d) {
    g.kT = d->kT; g.kH = d->kH; g.kW = d->kW;
    g.strT = d->sT; g.strH = d->sH; g.strW = d->sW;
    g.padT = d->pT; g.padH = d->pH; g.padW = d->pW;
    g.dilT = d->dT; g.dilH = d->dH; g.dilW = d->dW;
    g.fdkW = make_fastdiv(d->kW);
    g.fdkH = make_fastdiv(d->kH);
    g.fdsT = make_fastdiv(d->sT);
    g.fdsH = make_fastdiv(d->sH);
    g.fdsW = make_fastdiv(d->sW);
    g.scale = nullptr; g.shift = nullptr; g.relu = 0;
    g.fdHW = make_fastdiv((uint32_t)d->Hi * (uint32_t)d->Wi);
}
// 1x1x1 / (kT,1,1) convolutions with unit strides: input and output share (H, W)
static bool is_pointwise(const sf_conv_desc* d) {
    return d->kH == 1 && d->kW == 1 && d->sT == 1 && d->sH == 1 && d->sW == 1 && d->pH == 0 && d->pW == 0 &&
           d->Ho == d->Hi && d->Wo == d->Wi;
}

// gathered forward input: rows = output positions
static GatherSide gather_fwd(const sf_conv_desc* d, const void* x, const float* sc, const float* sh, int relu) {
    GatherSide g;
    memset(&g, 0, sizeof(g));
    fill_gather_common(g, d);
    g.src = (const f16*)x; g.ld = d->ldx; g.C = d->Ci;
    g.sT = d->Ti; g.sH = d->Hi; g.sW = d->Wi;
    g.mode = 0;
    g.Ktot = d->kT * d->kH * d->kW * d->Ci;
    g.fdC = make_fastdiv(d->Ci);
    g.fdrW = make_fastdiv(d->Wo); g.fdrH = make_fastdiv(d->Ho); g.fdrT = make_fastdiv(d->To);
    g.rowT = d->To;
    g.scale = sc; g.shift = sh; g.relu = relu;
    return g;
}
// gathered output gradient: rows = input positions
static GatherSide gather_dgrad(const sf_conv_desc* d, const void* dy) {
    GatherSide g;
    memset(&g, 0, sizeof(g));
    fill_gather_common(g, d);
    g.src = (const f16*)dy; g.ld = d->ldy; g.C = d->Co;
    g.sT = d->To; g.sH = d->Ho; g.sW = d->Wo;
    g.mode = 1;
    g.Ktot = d->kT * d->kH * d->kW * d->Co;
    g.fdC = make_fastdiv(d->Co);
    g.fdrW = make_fastdiv(d->Wi); g.fdrH = make_fastdiv(d->Hi); g.fdrT = make_fastdiv(d->Ti);
    g.rowT = d->Ti;
    return g;
}

// direct global -> LDS operand copies (GL): plain row-major GEMM operands only -- one tap, no fused input BatchNorm,
// K a multiple of the 32-wide K step, 16-byte aligned rows.  SF_IGEMM_GLDS=0 keeps the register-staged loads.
static bool igemm_glds_ok(const IgemmParams& p, bool pw) {
    static const bool off = tune_knob("SF_IGEMM_GLDS", 1) == 0;
    if (off || !pw || p.g.scale) return false;
    if (p.g.Ktot != p.g.C || p.g.Ktot % 32 != 0 || p.g.ld % 8 != 0 || p.ldw % 8 != 0) return false;
    if (p.g.padT != 0) return false;
    if (((uintptr_t)p.g.src | (uintptr_t)p.wmat) & 15) return false;
    if (p.bh > 0 && ((p.sa_b | p.sa_h | p.sw_b | p.sw_h) & 7)) return false;
    return true;
}

// SF_TRACE is read on every call (a getenv per launch is noise): tests switch it on mid-process
static inline bool sf_trace() { return test_hook("SF_TRACE", 0) != 0; }

// ------------------------------------------------------------------------------------------------
// One plan per implicit-GEMM pass (convolution forward / data gradient, Linear, batched GEMM): plan_gemm alone decides, launch_gemm
// launches what the plan says.  GEMM_GEN1: sf_igemm.h.  GEMM_GEN2: sf_igemm2.h, taken when the contraction is deep enough to pay for a
// 256-row tile with a three-stage direct-to-LDS pipeline; SF_IGEMM2=0 disables it, SF_IGEMM2_MINK sets the smallest K (default 512).
// GEMM_GEN2_CLASSES: that kernel, one launch per stride-residue class of a strided data gradient (igemm2_class).
enum GemmKind { GEMM_GEN1, GEMM_GEN2, GEMM_GEN2_CLASSES };
struct GemmPlan {
    GemmKind kind;
    bool pw;            // 1x1 taps with unit strides: rows are read without the gather
    int nbatch;
    int bn, bk;         // column tile 16 / 32 / 64 / 128; K step (second generation: 32 / 64, per class for GEMM_GEN2_CLASSES)
    bool t128;          // second generation: the `linear` 128 x 128 tile (it always steps 32)
    bool glds, cap;     // first generation: direct global -> LDS operand copies, 128-VGPR cap
    bool rows32;        // the variant that also writes fp32 side rows (sf_gemm_rows32: plain [M, K] operands)
    int bm;             // rows per M tile (= rows one bnb_part / column-sum row covers); 0 for the residue-class launches
};
// Second-generation K step and `linear` tile for M rows.  K step: 64 deep (48 KB stages, ONE 8-wave workgroup per CU) when the grid is at most ~one tile per CU anyway -- the
// res5-sized layers; otherwise 32 deep (24 KB stages, TWO workgroups per CU: one tile's epilogue and pipeline fill hide
// behind the other's K loop).  Measured per layer in profiles/r2/r2_v3_igemm2_variants.md.  SF_IGEMM2_BK=32|64 forces one.
static void plan_gemm2_tile(GemmPlan& g, const IgemmParams& p, int M) {
    const int tiles = cdiv(M, 256) * cdiv(p.Nout, p.Nout > 64 ? 128 : 64);
    const int force_bk = tune_knob("SF_IGEMM2_BK", 0);
    const bool bk64 = p.g.C % 64 == 0 && force_bk != 32 && (force_bk == 64 || tiles <= 320);
    g.bk = bk64 ? 64 : 32;
    // (256 x 256 tiles -- 128 flop per copied operand byte instead of 85, one workgroup per CU -- were measured in round 4 and
    // lost on both models: SlowFast 766.5 -> 741 clips/s on every eligible layer, 755 restricted to grids of >= 512 tiles,
    // MViTv2-S 590.9 -> 584 / 588; profiles/r4/r4_v6_knobs_ab.txt.  The same tile on a 16-wave workgroup (64 x 64 wave tiles, four
    // waves per SIMD kept) moved no layer either: profiles/r4/r4_v11_igemm2_fat_ab.txt.  Both removed.)
    // (A third-generation kernel -- sf_igemm3.h, 256 x 256 x 64 tiles on the eight-phase ping-pong schedule, 958-1013 TFLOP/s on
    // res5 a -- lived here as an opt-in through round 5.  Re-measured in the step with every threshold in round 6 it loses on both
    // models (SlowFast 855.7 vs 846.7 / 852.2 at >= 400 / 1500 tiles, MViTv2-S 739.4 vs 727.5 / 737.1: profiles/r6_v19_igemm3_instep_ab.txt):
    // one workgroup per CU leaves its HBM-bound epilogue uncovered.  Removed; commit 488e9e9 has the file and its tests.)
    // 128 x 128 tiles on four waves, THREE workgroups per CU (52 KB of LDS each), for the plain matrix products (`linear`) without a statistics / column-sum
    // epilogue whose grid is several rounds deep anyway (the MViT Linears with K >= 512: fc2, the fc1 / qkv data gradients): a third
    // resident workgroup hides more of the store epilogue than the bigger tile saves in operand traffic -- fc2 forward 103.7 ->
    // 99.2 us HBM-cold, MViTv2-S 707 -> 712 clips/s (profiles/r5_v35_*).  Not below K = 512 (there the round-1 kernel at four
    // workgroups per CU stays ahead: 114 vs 128 us for fc1).
    const int t128 = test_hook("SF_IGEMM2_T128", 1);      // 2: also on grids of at most one round (tests)
    g.t128 = t128 && p.linear && p.Nout > 64 && !p.stat_part && !p.bnb_part && (!bk64 || t128 == 2);
}
static bool igemm2_operands_ok(const IgemmParams& p, int nbatch) {
    const GatherSide& g = p.g;
    if (nbatch != 1 || g.scale) return false;
    if (p.bh > 1 || (p.bh == 1 && (p.sa_b | p.sa_h | p.sw_b | p.sw_h | p.sy_b | p.sy_h | p.sr_b | p.sr_h))) return false;
    const int taps = g.kT * g.kH * g.kW;
    if (taps > SF_I2_MAXTAPS || g.C % 32 != 0 || g.Ktot != taps * g.C) return false;
    if (g.ld % 8 != 0 || p.ldw % 8 != 0 || p.ldw < g.Ktot) return false;
    if (((uintptr_t)g.src | (uintptr_t)p.wmat) & 15) return false;
    if ((g.kT - 1) * g.dilT > 127 || (g.kH - 1) * g.dilH > 127 || (g.kW - 1) * g.dilW > 127) return false;
    return true;
}
static void igemm2_common(Igemm2Params& q, const IgemmParams& p) {
    const GatherSide& g = p.g;
    memset(&q, 0, sizeof(q));
    q.src = g.src; q.ld = g.ld; q.C = g.C;
    q.sT = g.sT; q.sH = g.sH; q.sW = g.sW;
    q.wmat = p.wmat; q.ldw = p.ldw; q.Nout = p.Nout;
    q.y = p.y; q.ldy = p.ldy; q.bias = p.bias; q.resid = p.resid; q.ldr = p.ldr; q.stat_part = p.stat_part;
    q.act_mode = p.act_mode; q.act_aux = p.act_aux; q.ld_aux = p.ld_aux; q.resid_row0 = p.resid_row0; q.alpha = p.alpha;
    q.resid_bits = p.resid_bits;
    q.bnb_y = p.bnb_y; q.bnb_ld = p.bnb_ld; q.bnb_scale = p.bnb_scale; q.bnb_shift = p.bnb_shift; q.bnb_part = p.bnb_part;
    q.bnb_bits = p.bnb_bits;
    q.f32 = p.f32;
    q.linear = p.linear;
    q.ablate = tune_knob("SF_IGEMM2_ABLATE", 0);        // diagnostic builds only: parts of the kernel switched off (wrong results)
}
// GEMM_GEN2: every row, every tap
static void igemm2_dense(Igemm2Params& q, const IgemmParams& p) {
    const GatherSide& g = p.g;
    igemm2_common(q, p);
    q.fdrW = g.fdrW; q.fdrH = g.fdrH; q.fdrT = g.fdrT;
    const int sgn = g.mode == 0 ? 1 : -1;
    if (g.mode == 0) {
        q.mulT = g.strT; q.mulH = g.strH; q.mulW = g.strW;
        q.offT = -g.padT; q.offH = -g.padH; q.offW = -g.padW;
    } else {
        q.mulT = q.mulH = q.mulW = 1;
        q.offT = g.padT; q.offH = g.padH; q.offW = g.padW;
    }
    q.ntaps = g.kT * g.kH * g.kW;
    int t = 0;
    for (int kt = 0; kt < g.kT; ++kt)
        for (int kh = 0; kh < g.kH; ++kh)
            for (int kw = 0; kw < g.kW; ++kw, ++t) {
                const int dt = sgn * kt * g.dilT, dh = sgn * kh * g.dilH, dw = sgn * kw * g.dilW;
                q.dt[t] = (int8_t)dt; q.dh[t] = (int8_t)dh; q.dw[t] = (int8_t)dw;
                q.taps[t].dlin = (dt * g.sH + dh) * g.sW + dw;
                q.taps[t].wcol = t * g.C;
            }
    q.M = p.M;
}

// Strided data gradient as sub-convolutions (reference op: the backward of nn.Conv3d with stride > 1 -- ResBlock.branch1
// and BottleneckTransform.b at the first block of a stage, resnet_helper.py:346-358, 485-493; FuseFastToSlow.conv_f2s,
// video_model_builder.py:147-154).  dx[i] = sum over the taps k with (i + pad - k*dil) divisible by the stride of
// dy[(i + pad - k*dil) / stride] . w[k]: input positions of one residue class r = (i + pad) mod stride share their tap set,
// and inside a class both the source position and the output position are affine in the class coordinates.  One launch
// per class: no all-padding K steps (a 3x3 stride-2 convolution wastes 3/4 of them in the gather formulation, a strided
// 1x1 shortcut 3/4 of its ROWS), every tap of a step real, wave-uniform and direct-to-LDS.  Classes without any tap
// (1x1 kernels) just store the residual / zeros.
// GEMM_GEN2_CLASSES: the launch of residue class r; false when the class holds no input position
static bool igemm2_class(Igemm2Params& q, const IgemmParams& p, const int r[3]) {
    const GatherSide& g = p.g;
    const int Ti = (int)g.fdrT.d, Hi = (int)g.fdrH.d, Wi = (int)g.fdrW.d;      // rows = input positions
    const int N = p.M / (Ti * Hi * Wi);
    const int str[3] = {g.strT, g.strH, g.strW}, pad[3] = {g.padT, g.padH, g.padW}, dil[3] = {g.dilT, g.dilH, g.dilW};
    const int ker[3] = {g.kT, g.kH, g.kW}, ext[3] = {Ti, Hi, Wi};
    int q0[3], cnt[3];
    for (int a = 0; a < 3; ++a) {
        const int num = pad[a] - r[a];
        q0[a] = num > 0 ? (num + str[a] - 1) / str[a] : 0;
        const int top = ext[a] - 1 + pad[a] - r[a];
        const int q1 = top >= 0 ? top / str[a] : -1;
        cnt[a] = q1 - q0[a] + 1;
        if (cnt[a] <= 0) return false;
    }
    igemm2_common(q, p);
    q.fdrT = make_fastdiv(cnt[0]); q.fdrH = make_fastdiv(cnt[1]); q.fdrW = make_fastdiv(cnt[2]);
    q.mulT = q.mulH = q.mulW = 1;
    q.offT = q0[0]; q.offH = q0[1]; q.offW = q0[2];
    int nt = 0, tap = 0;
    for (int kt = 0; kt < ker[0]; ++kt)
        for (int kh = 0; kh < ker[1]; ++kh)
            for (int kw = 0; kw < ker[2]; ++kw, ++tap) {
                const int k[3] = {kt, kh, kw};
                int d[3];
                bool ok = true;
                for (int a = 0; a < 3; ++a) {
                    const int v = r[a] - k[a] * dil[a];
                    if (v % str[a] != 0) { ok = false; break; }
                    d[a] = v / str[a];
                }
                if (!ok) continue;
                q.dt[nt] = (int8_t)d[0]; q.dh[nt] = (int8_t)d[1]; q.dw[nt] = (int8_t)d[2];
                q.taps[nt].dlin = (d[0] * g.sH + d[1]) * g.sW + d[2];
                q.taps[nt].wcol = tap * g.C;
                ++nt;
            }
    q.ntaps = nt;
    q.M = N * cnt[0] * cnt[1] * cnt[2];
    q.omap = 1;
    q.oT = Ti; q.oH = Hi; q.oW = Wi;
    q.omT = str[0]; q.omH = str[1]; q.omW = str[2];
    q.ooT = str[0] * q0[0] + r[0] - pad[0]; q.ooH = str[1] * q0[1] + r[1] - pad[1]; q.ooW = str[2] * q0[2] + r[2] - pad[2];
    return true;
}

static GemmPlan plan_gemm(const IgemmParams& p, bool pointwise, int nbatch) {
    GemmPlan g;
    memset(&g, 0, sizeof(g));
    g.pw = pointwise; g.nbatch = nbatch; g.rows32 = p.f32.out != nullptr;
    g.bn = p.Nout > 64 ? 128 : p.Nout > 32 ? 64 : p.Nout > 16 ? 32 : 16;   // the second generation has no 16, and 32 for residue classes only
    // hooks are read on every call (a few getenv per launch are noise): tests lower the thresholds for single cases
    const bool gen2 = test_hook("SF_IGEMM2", 1) != 0 && p.M >= test_hook("SF_IGEMM2_MINROWS", 4096) && igemm2_operands_ok(p, nbatch);
    const bool unit = p.g.strT == 1 && p.g.strH == 1 && p.g.strW == 1;
    if (gen2 && p.g.Ktot >= test_hook("SF_IGEMM2_MINK", 512) && p.Nout > 32 && (p.g.mode == 0 || unit)) {
        g.kind = GEMM_GEN2;
        plan_gemm2_tile(g, p, p.M);
        g.bm = g.t128 ? 128 : 256;
        return g;
    }
    if (gen2 && tune_knob("SF_IGEMM2_STRIDED", 1) != 0 && p.g.mode == 1 && !unit && p.Nout > 16 && !p.stat_part && !p.act_mode) {
        g.kind = GEMM_GEN2_CLASSES;     // bk: launch_gemm, per class; bm stays 0
        return g;
    }
    g.kind = GEMM_GEN1;
    g.bk = 32; g.bm = 128;
    g.glds = igemm_glds_ok(p, pointwise);
    // 128-VGPR cap (4 workgroups per CU) for the 128-wide tile: +0.2..1.2 % end to end (profiles/r1_visit9_*_occ4.json);
    // SF_IGEMM_OCC4=0 restores the uncapped build for A/B runs (the direct-to-LDS and side-row variants exist capped only)
    static const bool occ4 = tune_knob("SF_IGEMM_OCC4", 1) != 0;
    g.cap = g.bn == 128 && (occ4 || g.glds || g.rows32);
    return g;
}

template <int BN, int WM, int WN>
static void launch_igemm(const GemmPlan& g, IgemmParams& p, hipStream_t s) {
    p.ntiles_n = cdiv(p.Nout, BN);
    const dim3 grid((unsigned)(cdiv(p.M, 128) * p.ntiles_n), (unsigned)g.nbatch), block(SF_THREADS);
    constexpr bool kCap = BN == 128;        // 128-VGPR cap only matters (and is only compiled) for the 128-wide tile
    if (g.rows32) {
        if (g.glds) hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, true, true, kCap, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, true, false, kCap, true>), grid, block, 0, s, p);
    } else if (g.glds) {
        hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, true, true, kCap>), grid, block, 0, s, p);
    } else if (g.pw) {
        if (g.cap) hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, true, false, kCap>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, true, false, false>), grid, block, 0, s, p);
    } else {
        if (g.cap) hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, false, false, kCap>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((sf_igemm_kernel<BN, WM, WN, false, false, false>), grid, block, 0, s, p);
    }
}
template <int BM, int BN, int BK>           // 256 x BN tiles on 4 x 2 waves, 128 x 128 on 2 x 2
static void launch_igemm2(const GemmPlan& g, Igemm2Params& q, hipStream_t s) {
    constexpr int WM = BM / 64;
    q.ntiles_n = cdiv(q.Nout, BN);
    const dim3 grid((unsigned)(cdiv(q.M, BM) * q.ntiles_n)), block(WM * 128);
    if constexpr (BN >= 64) {       // (N <= 32 never reaches this kernel densely: plan_gemm)
        if (g.rows32) { hipLaunchKernelGGL((sf_igemm2_kernel<BM, BN, WM, 2, BK, 3, true>), grid, block, 0, s, q); return; }
    }
    hipLaunchKernelGGL((sf_igemm2_kernel<BM, BN, WM, 2, BK, 3>), grid, block, 0, s, q);
}
static void launch_gemm2(const GemmPlan& g, Igemm2Params& q, hipStream_t s) {
    if (sf_trace()) fprintf(stderr, "[sfamd] igemm2: M=%d N=%d C=%d taps=%d BK=%d omap=%d\n", q.M, q.Nout, q.C, q.ntaps, g.bk, q.omap);
    if (g.t128) launch_igemm2<128, 128, 32>(g, q, s);
    else if (g.bn == 128) { if (g.bk == 64) launch_igemm2<256, 128, 64>(g, q, s); else launch_igemm2<256, 128, 32>(g, q, s); }
    else if (g.bn == 64) { if (g.bk == 64) launch_igemm2<256, 64, 64>(g, q, s); else launch_igemm2<256, 64, 32>(g, q, s); }
    else launch_igemm2<256, 32, 32>(g, q, s);
}
// The one switch over the kernel instantiations of the family (p.ntiles_n is the launcher's to write)
static void launch_gemm(const GemmPlan& g, IgemmParams& p, hipStream_t s) {
    Igemm2Params q;
    switch (g.kind) {
    case GEMM_GEN2: igemm2_dense(q, p); launch_gemm2(g, q, s); return;
    case GEMM_GEN2_CLASSES:
        for (int rt = 0; rt < p.g.strT; ++rt)
            for (int rh = 0; rh < p.g.strH; ++rh)
                for (int rw = 0; rw < p.g.strW; ++rw) {
                    const int r[3] = {rt, rh, rw};
                    if (!igemm2_class(q, p, r)) continue;
                    GemmPlan gc = g;
                    plan_gemm2_tile(gc, p, q.M);
                    launch_gemm2(gc, q, s);
                }
        return;
    case GEMM_GEN1:
        if (g.bn == 128) launch_igemm<128, 64, 64>(g, p, s);
        else if (g.bn == 64) launch_igemm<64, 32, 64>(g, p, s);
        else if (g.bn == 32) launch_igemm<32, 32, 32>(g, p, s);
        else launch_igemm<16, 32, 16>(g, p, s);
        return;
    }
}
// plan + launch of a convolution pass; the plan goes back to callers that need the rows per M tile
static int run_igemm(IgemmParams& p, bool pw, hipStream_t s, GemmPlan* plan = nullptr) {
    const GemmPlan g = plan_gemm(p, pw, 1);
    if (plan) *plan = g;
    launch_gemm(g, p, s);
    return check_launch(g.kind == GEMM_GEN2 ? "igemm2" : g.kind == GEMM_GEN2_CLASSES ? "igemm2 strided dgrad" : "igemm");
}

// ------------------------------------------------------------------------------------------------
// LDS-patch direct convolution for the thin W-pair-folded stems (sf_stem.h); SF_STEM_GENERIC=1 keeps the implicit GEMM.
enum StemFwd { STEM_FWD_GENERIC, STEM_FWD_SMALL_GENERIC, STEM_FWD_SMALL_ROWS_1_3, STEM_FWD_ROWS_2_7, STEM_FWD_SLIDE };
struct StemPlan {
    bool ok, thin3, small;      // small: the patch fits SF_STEM_CHUNKS_SMALL (12 KiB of LDS instead of 52)
    int tiles_w, tiles_h, tiles_t, ntiles, F, PR;
    int wg_blocks, tiles_per_block, Kpad, wgroups;
    size_t ws_bytes;
    StemFwd fwd;                // plan_stem_fwd: the forward kernel variant ...
    int seg_groups;             // ... and, for STEM_FWD_SLIDE, the groups of 4 output frames one workgroup walks
};
static StemPlan plan_stem(const sf_conv_desc* d) {
    StemPlan s;
    memset(&s, 0, sizeof(s));
    static const bool off = tune_knob("SF_STEM_GENERIC", 0) != 0;
    if (off) return s;
    // thin3: an 8-channel (kT, kH, 3) stride-1 layer with one pixel of W padding (the Fast pathway's res2 1x3x3 bottleneck) is the
    // same direct convolution with a zero fourth tap: forward, data gradient (conv_dgrad_impl) and weight gradient.  Measured on
    // s2.fast b (profiles/r3/r3_v13_thin3_ab.txt): fwd 105 -> 57-69 us, dgrad 110 -> 56, wgrad 95 -> 90; SlowFast step +0.6 %.
    // SF_STEM_THIN3=0 keeps the implicit GEMM for A/B runs.
    static const bool thin3_on = tune_knob("SF_STEM_THIN3", 1) != 0;
    const bool stemlike = d->kW == 4 && d->pW == 2;
    const bool thin3 = thin3_on && d->kW == 3 && d->pW == 1 && d->sH == 1 && d->sT == 1;
    if (d->Ci != 8 || d->Cw != 8 || !(stemlike || thin3) || d->sW != 1 || d->dT != 1 || d->dH != 1 || d->dW != 1)
        return s;
    s.thin3 = thin3;
    if (d->Co > 16 || d->Co % 8 != 0 || (d->Cow && d->Cow != d->Co)) return s;
    if (d->kT * d->kH > SF_STEM_MAX_SLICES) return s;
    s.F = (SF_STEM_TT - 1) * d->sT + d->kT;
    s.PR = (SF_STEM_TH - 1) * d->sH + d->kH;
    if ((int64_t)s.F * s.PR * SF_STEM_PC > SF_STEM_CHUNKS) return s;
    s.small = (int64_t)s.F * s.PR * SF_STEM_PC <= SF_STEM_CHUNKS_SMALL;
    s.tiles_w = cdiv(d->Wo, SF_STEM_TW);
    s.tiles_h = cdiv(d->Ho, SF_STEM_TH);
    s.tiles_t = cdiv(d->To, SF_STEM_TT);
    const int64_t nt = (int64_t)d->N * s.tiles_t * s.tiles_h * s.tiles_w;
    if (nt >= (1ll << 30)) return s;
    s.ntiles = (int)nt;
    const int gmax = s.small ? 1024 : 512;               // persistent 8-wave workgroups: 2 per CU (52 KiB patches), 4 with small ones
    int g = s.ntiles < gmax ? s.ntiles : gmax;
    s.tiles_per_block = cdiv(s.ntiles, g);
    s.wg_blocks = cdiv(s.ntiles, s.tiles_per_block);
    s.Kpad = roundup(d->kT * d->kH * 32, 128);
    { const int nsl = d->kT * d->kH; s.wgroups = nsl <= 4 ? 8 / nsl : 1; }      // sf_stem_wgrad_kernel: wave groups share a tile's rows
    s.ws_bytes = (size_t)s.wg_blocks * s.wgroups * 16 * s.Kpad * 4;
    s.ok = true;
    return s;
}
// SF_STEM_SLIDE (test hook, read per call): groups of 4 output frames a workgroup of the sliding Fast-stem forward walks; 0 = the
// tile kernel.  profiles/r6_v34_stem_slide_ab.txt
#define SF_STEM_SLIDE_GROUPS 4
// The direct convolution as a forward-shaped pass (forward, fused forward, thin3 data gradient): plan_stem plus the kernel variant.
// !ok, the implicit GEMM runs: d is no stem (no thin3 layer with `thin3_only`), or the tiles outnumber the `table_rows` rows of the
// partial table they fill (`table`: statistics or the fused BatchNorm-backward sums, `bnb`).  Variants: patch-row-major for the two
// shapes that matter (row stride / kernel height compile-time), generic loop otherwise; SF_STEM_ROWMAJOR=0 keeps the generic loop
static StemPlan plan_stem_fwd(const sf_conv_desc* d, bool thin3_only, bool table, int table_rows, bool bnb) {
    StemPlan s = plan_stem(d);
    if (!s.ok || (thin3_only && !s.thin3) || (table && s.ntiles > table_rows)) { s.ok = false; return s; }
    static const bool rm = tune_knob("SF_STEM_ROWMAJOR", 1) != 0;
    const int sg = test_hook("SF_STEM_SLIDE", SF_STEM_SLIDE_GROUPS);
    const bool rows_2_7 = rm && d->sH == 2 && d->kH == 7 && !s.small;
    if (rows_2_7 && sg > 0 && d->sT == 1 && d->kT > 1 && d->kT <= 5 && d->Co <= 8 && !bnb) {
        s.fwd = STEM_FWD_SLIDE;
        s.seg_groups = sg < s.tiles_t ? sg : s.tiles_t;
    } else if (rows_2_7) s.fwd = STEM_FWD_ROWS_2_7;
    else if (rm && d->sH == 1 && d->kH == 3 && s.small) s.fwd = STEM_FWD_SMALL_ROWS_1_3;
    else s.fwd = s.small ? STEM_FWD_SMALL_GENERIC : STEM_FWD_GENERIC;
    return s;
}
static void launch_stem_fwd(const StemPlan& sp, const StemParams& q, hipStream_t s) {
    const dim3 g(sp.ntiles), b(SF_THREADS);
    switch (sp.fwd) {
    case STEM_FWD_SLIDE: {
        StemParams qs = q;                   // a workgroup walks seg_groups groups of 4 output frames (sf_stem_fwd_slide_kernel)
        qs.seg_groups = sp.seg_groups; qs.tiles_t = cdiv(sp.tiles_t, qs.seg_groups); qs.fd_tt = make_fastdiv(qs.tiles_t);
        const dim3 gs((unsigned)((int64_t)q.N * qs.tiles_t * sp.tiles_h * sp.tiles_w));
        if (sf_trace()) fprintf(stderr, "[sfamd] stem_fwd_slide: %u runs of %d groups\n", gs.x, qs.seg_groups);
        hipLaunchKernelGGL((sf_stem_fwd_slide_kernel<2, 7>), gs, b, 0, s, qs);
        return;
    }
    case STEM_FWD_ROWS_2_7: hipLaunchKernelGGL((sf_stem_fwd_kernel<SF_STEM_CHUNKS, 2, 7>), g, b, 0, s, q); return;
    case STEM_FWD_SMALL_ROWS_1_3: hipLaunchKernelGGL((sf_stem_fwd_kernel<SF_STEM_CHUNKS_SMALL, 1, 3>), g, b, 0, s, q); return;
    case STEM_FWD_SMALL_GENERIC: hipLaunchKernelGGL((sf_stem_fwd_kernel<SF_STEM_CHUNKS_SMALL>), g, b, 0, s, q); return;
    case STEM_FWD_GENERIC: hipLaunchKernelGGL((sf_stem_fwd_kernel<SF_STEM_CHUNKS>), g, b, 0, s, q); return;
    }
}
static StemParams stem_params(const sf_conv_desc* d, const StemPlan& s, const void* x) {
    StemParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const f16*)x; p.ldx = d->ldx;
    p.N = d->N; p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi;
    p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo; p.Co = d->Co;
    p.kT = d->kT; p.kH = d->kH; p.sT = d->sT; p.sH = d->sH; p.pT = d->pT; p.pH = d->pH;
    p.pW = d->pW;
    if (s.thin3) { p.wo0 = 0; p.wos = 24; p.wog = 8; p.kwc = 3; }
    else { p.wo0 = 0; p.wos = 32; p.wog = 8; p.kwc = 4; }
    p.ldy = d->ldy;
    p.tiles_w = s.tiles_w; p.tiles_h = s.tiles_h; p.tiles_t = s.tiles_t; p.ntiles = s.ntiles;
    p.fd_tw = make_fastdiv(s.tiles_w); p.fd_th = make_fastdiv(s.tiles_h); p.fd_tt = make_fastdiv(s.tiles_t);
    p.F = s.F; p.PR = s.PR;
    p.fd_pc = make_fastdiv(SF_STEM_PC); p.fd_prpc = make_fastdiv(s.PR * SF_STEM_PC);
    p.Kpad = s.Kpad; p.tiles_per_block = s.tiles_per_block; p.wgroups = s.wgroups;
    return p;
}
static StemParams stem_fwd_params(const sf_conv_desc* d, const StemPlan& s, const void* x, const void* w, int ldw, void* y) {
    StemParams p = stem_params(d, s, x);
    p.wmat = (const f16*)w; p.ldw = ldw; p.y = (f16*)y;
    return p;
}
// the operands every implicit-GEMM pass has: gathered rows x packed weights -> 16-bit rows, optional bias and residual
static IgemmParams gemm_params(const GatherSide& g, int M, const void* w, int ldw, int Nout, void* y, int ldy,
                               const float* bias, const void* resid, int ldr) {
    IgemmParams p;
    memset(&p, 0, sizeof(p));
    p.g = g; p.M = M; p.ksteps = cdiv(g.Ktot, 32);
    p.wmat = (const f16*)w; p.ldw = ldw; p.Nout = Nout; p.y = (f16*)y; p.ldy = ldy;
    p.bias = bias; p.resid = (const f16*)resid; p.ldr = ldr;
    return p;
}

extern "C" int sf_conv_weight_ld(const sf_conv_desc* d, int32_t* ldf, int32_t* ldd) {
    REQUIRE(d && ldf && ldd, "sf_conv_weight_ld: null argument");
    int taps = d->kT * d->kH * d->kW;
    *ldf = roundup(taps * d->Ci, 32);
    *ldd = roundup(taps * d->Co, 32);
    return 0;
}

static PrepParams prep_params(const sf_conv_desc* d, const float* w, void* wf, void* wd) {
    PrepParams p;
    memset(&p, 0, sizeof(p));
    p.w = w; p.Co = d->Co; p.Cow = d->Cow ? d->Cow : d->Co; p.Cw = d->Cw; p.Cp = d->Ci; p.taps = d->kT * d->kH * d->kW;
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    p.wf = (f16*)wf; p.ldf = ldf; p.wd = (f16*)wd; p.ldd = ldd;
    return p;
}

extern "C" int sf_prep_weights(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(w && wf, "sf_prep_weights: null pointer");
    const PrepParams p = prep_params(d, w, wf, wd);
    int64_t total = (int64_t)p.Co * p.ldf + (wd ? (int64_t)p.Cp * p.ldd : 0);
    int blocks = (int)((total + SF_THREADS - 1) / SF_THREADS);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sf_prep_weights_kernel, dim3(blocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("prep_weights");
}

static_assert(sizeof(sf_prep_item) == sizeof(PrepParams), "sf_prep_item must mirror PrepParams");
extern "C" int sf_prep_item_fill(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_prep_item* item) {
    if (check_desc(d)) return -1;
    REQUIRE(w && wf && item, "sf_prep_item_fill: null pointer");
    PrepParams p = prep_params(d, w, wf, wd);
    p.pad = sf_prep_tile_co(p.taps);
    memcpy(item, &p, sizeof(p));
    return 0;
}

extern "C" int64_t sf_prep_item_blocks(const sf_prep_item* item) {
    REQUIRE(item && item->Co > 0 && item->ldf > 0 && item->taps > 0, "sf_prep_item_blocks: bad item");
    REQUIRE(item->pad == sf_prep_tile_co(item->taps), "sf_prep_item_blocks: item was not written by sf_prep_item_fill");
    if (item->pad > 0) return (int64_t)cdiv(item->Co, item->pad) * cdiv(item->Cp, SF_PREP_TILE_CI);
    const int64_t n = (int64_t)item->Co * item->ldf + (item->wd ? (int64_t)item->Cp * item->ldd : 0);
    return cdiv(n, SF_PREP_BLOCK_ELEMS);
}

extern "C" int sf_prep_weights_batch(const sf_prep_item* items, const int32_t* blk_item, const int32_t* blk_off,
                                     int32_t nblocks, sf_stream_t stream) {
    REQUIRE(items && blk_item && blk_off && nblocks > 0, "sf_prep_weights_batch: bad arguments");
    hipLaunchKernelGGL(sf_prep_weights_batch_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream,
                       (const PrepParams*)items, blk_item, blk_off);
    return check_launch("prep_weights_batch");
}

extern "C" int sf_conv_fwd_mtiles(const sf_conv_desc* d) {
    if (!d) return fail("sf_conv_fwd_mtiles: null descriptor");
    return cdiv((int64_t)d->N * d->To * d->Ho * d->Wo, 128);
}

extern "C" int sf_conv_fwd(const sf_conv_desc* d, const void* x, const void* wf, const float* in_scale,
                           const float* in_shift, int in_relu, const float* bias, void* y, float* stat_part,
                           sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(x && wf && y, "sf_conv_fwd: null pointer");
    REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "sf_conv_fwd: in_scale/in_shift must come together");
    REQUIRE(!in_scale || d->Ci <= 512, "sf_conv_fwd: fused input BatchNorm supports Ci <= 512 (got %d)", d->Ci);
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    if (!in_scale && !bias) {
        const StemPlan sp = plan_stem_fwd(d, false, stat_part != nullptr, sf_conv_fwd_mtiles(d), false);
        if (sp.ok) {
            StemParams q = stem_fwd_params(d, sp, x, wf, ldf, y);
            q.stat_part = stat_part; q.stat_rows = sf_conv_fwd_mtiles(d);
            if (sf_trace()) fprintf(stderr, "[sfamd] stem_fwd: %d tiles, patch %dx%dx%d chunks\n", sp.ntiles, sp.F, sp.PR, SF_STEM_PC);
            launch_stem_fwd(sp, q, (hipStream_t)stream);
            return check_launch("stem_fwd");
        }
    }
    IgemmParams p = gemm_params(gather_fwd(d, x, in_scale, in_shift, in_relu), d->N * d->To * d->Ho * d->Wo, wf, ldf, d->Co,
                                y, d->ldy, bias, nullptr, 0);
    p.stat_part = stat_part;
    return run_igemm(p, is_pointwise(d), (hipStream_t)stream);
}

extern "C" int sf_conv_fwd_fused(const sf_conv_desc* d, const void* x, const void* wf, const float* bias,
                                 const void* resid, int32_t ldr, int out_relu, void* y, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(x && wf && y, "sf_conv_fwd_fused: null pointer");
    REQUIRE(!resid || (ldr >= d->Co && ldr % 8 == 0), "sf_conv_fwd_fused: bad residual pitch");
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    if (!resid) {        // thin W-pair-folded stems: the LDS-patch direct convolution with bias / ReLU in its epilogue
        const StemPlan sp = plan_stem_fwd(d, false, false, 0, false);
        if (sp.ok) {
            StemParams q = stem_fwd_params(d, sp, x, wf, ldf, y);
            q.bias = bias; q.out_relu = out_relu;
            launch_stem_fwd(sp, q, (hipStream_t)stream);
            return check_launch("stem_fwd_fused");
        }
    }
    IgemmParams p = gemm_params(gather_fwd(d, x, nullptr, nullptr, 0), d->N * d->To * d->Ho * d->Wo, wf, ldf, d->Co,
                                y, d->ldy, bias, resid, ldr);
    p.act_mode = out_relu ? 3 : 0;
    return run_igemm(p, is_pointwise(d), (hipStream_t)stream);
}

struct BnFuse {     // the fused BatchNorm-backward reduction of sf_conv_dgrad_bn (all device pointers)
    const float* scale; const float* shift; const void* bits;
    const void* y0; int32_t ld0; float* part0;
};
static int conv_dgrad_impl(const sf_conv_desc* d, const void* dy, const void* wd, const void* resid, int32_t ldr,
                           const void* resid_bits, void* dx, const BnFuse* bn, int32_t* bn_rows, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(dy && wd && dx, "sf_conv_dgrad: null pointer");
    REQUIRE(!resid || (ldr >= d->Ci && ldr % 8 == 0), "sf_conv_dgrad: bad residual pitch");
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    IgemmParams p = gemm_params(gather_dgrad(d, dy), d->N * d->Ti * d->Hi * d->Wi, wd, ldd, d->Ci, dx, d->ldx, nullptr, resid, ldr);
    REQUIRE(!resid_bits || resid, "sf_conv_dgrad: resid_bits without a residual");
    p.resid_bits = (const uint8_t*)resid_bits;
    // the fused BatchNorm-backward reduction rides on dense stride-1 data gradients only (a strided one runs as one launch
    // per residue class of input positions, or gathers with 3/4 of its taps masked): the caller then keeps sf_bn_bwd_reduce
    const bool fuse = bn && d->sT == 1 && d->sH == 1 && d->sW == 1;
    // thin3 (plan_stem): the data gradient of an 8-channel same-size (kT, kH, 3) layer is the LDS-patch direct convolution of dy
    // with the flipped kernel, read from the packed data-gradient operand in reverse order
    if (!resid && d->Co == 8 && d->To == d->Ti && d->Ho == d->Hi && d->Wo == d->Wi) {
        sf_conv_desc dd = *d;
        dd.Ci = d->Co; dd.Cw = d->Co; dd.Co = d->Ci; dd.Cow = 0;
        dd.pT = d->kT - 1 - d->pT; dd.pH = d->kH - 1 - d->pH; dd.pW = d->kW - 1 - d->pW;
        dd.ldx = d->ldy; dd.ldy = d->ldx;
        const StemPlan sp = plan_stem_fwd(&dd, true, fuse, cdiv(p.M, 128), fuse);
        if (sp.ok) {
            StemParams q = stem_fwd_params(&dd, sp, dy, wd, ldd, dx);
            const int S = d->kT * d->kH;
            q.wo0 = ((S - 1) * 3 + 2) * 8; q.wos = -24; q.wog = -8; q.kwc = 3;
            if (fuse) {
                q.bnb_y = (const f16*)bn->y0; q.bnb_ld = bn->ld0; q.bnb_scale = bn->scale; q.bnb_shift = bn->shift;
                q.bnb_bits = (const uint8_t*)bn->bits;
                q.stat_part = bn->part0; q.stat_rows = 0;
            }
            launch_stem_fwd(sp, q, (hipStream_t)stream);
            if (bn_rows) *bn_rows = fuse ? sp.ntiles : 0;
            return check_launch("stem_dgrad");
        }
    }
    if (fuse) {
        p.bnb_y = (const f16*)bn->y0; p.bnb_ld = bn->ld0; p.bnb_part = bn->part0;
        p.bnb_scale = bn->scale; p.bnb_shift = bn->shift; p.bnb_bits = (const uint8_t*)bn->bits;
    }
    GemmPlan g;
    const int rc = run_igemm(p, is_pointwise(d), (hipStream_t)stream, &g);
    if (bn_rows) *bn_rows = (fuse && g.bm > 0) ? cdiv(p.M, g.bm) : 0;
    return rc;
}

extern "C" int sf_conv_dgrad(const sf_conv_desc* d, const void* dy, const void* wd, const void* resid, int32_t ldr,
                             const void* resid_bits, void* dx, sf_stream_t stream) {
    return conv_dgrad_impl(d, dy, wd, resid, ldr, resid_bits, dx, nullptr, nullptr, stream);
}

extern "C" int sf_conv_dgrad_bn(const sf_conv_desc* d, const void* dy, const void* wd, const void* resid, int32_t ldr,
                                const void* resid_bits, void* dx, const float* mask_scale, const float* mask_shift,
                                const void* mask_bits, const void* bn_y, int32_t bn_ldy, float* bn_part, int32_t bn_part_rows,
                                int32_t* bn_rows, sf_stream_t stream) {
    REQUIRE(d && bn_y && bn_part && bn_rows, "sf_conv_dgrad_bn: null pointer");
    REQUIRE(mask_bits || (mask_scale && mask_shift), "sf_conv_dgrad_bn: a mask source is needed (mask_bits, or mask_scale + mask_shift)");
    REQUIRE(bn_ldy >= d->Ci && bn_ldy % 8 == 0 && ((uintptr_t)bn_y & 15) == 0, "sf_conv_dgrad_bn: bad bn_y pitch / alignment");
    REQUIRE((int64_t)bn_part_rows * 128 >= (int64_t)d->N * d->Ti * d->Hi * d->Wi,
            "sf_conv_dgrad_bn: the partial table needs ceil(positions / 128) rows of [2][Ci] floats");
    const BnFuse bn = {mask_scale, mask_shift, mask_bits, bn_y, bn_ldy, bn_part};
    return conv_dgrad_impl(d, dy, wd, resid, ldr, resid_bits, dx, &bn, bn_rows, stream);
}

// First-generation weight-gradient tiles (sf_conv_wgrad, sf_bgemm_tn): output rows in tiles of BMW, KS 32-position chunks per stage
static inline int wgrad1_bmw(int rows) { return rows >= 128 ? 128 : rows >= 64 ? 64 : rows >= 32 ? 32 : 16; }
static inline int wgrad1_ks(int bmw) { return bmw <= 32 ? 4 : 1; }
static void launch_wgrad1(int bmw, WgradParams& p, dim3 grid3, hipStream_t s) {
    p.tiles_k = grid3.x; p.tiles_c = grid3.y;
    const dim3 grid(grid3.x * grid3.y * grid3.z), block(SF_THREADS);
    switch (bmw) {
        case 128: hipLaunchKernelGGL((sf_wgrad_kernel<128, 64, 64, 1>), grid, block, 0, s, p); break;
        case 64: hipLaunchKernelGGL((sf_wgrad_kernel<64, 32, 64, 1>), grid, block, 0, s, p); break;
        case 32: hipLaunchKernelGGL((sf_wgrad_kernel<32, 32, 32, 4>), grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL((sf_wgrad_kernel<16, 16, 32, 4>), grid, block, 0, s, p); break;
    }
}
// sums `slabs` partial tile sets of [Co_pad][Kpad] into dw: ~>= 4 per lane, 8..256 element quads per block
static void launch_wgrad_reduce(const sf_conv_desc* d, const float* ws, int slabs, int Co_pad, int Kpad, bool slice4, float* dw,
                                float out_scale, int zero_first, hipStream_t s) {
    WgradReduceParams r;
    memset(&r, 0, sizeof(r));
    r.ws = ws; r.splits = slabs; r.Co = d->Cow ? d->Cow : d->Co; r.Co_pad = Co_pad; r.Kpad = Kpad;
    r.taps = d->kT * d->kH * d->kW; r.Ktot = r.taps * d->Ci; r.fdC = make_fastdiv(d->Ci); r.dw = dw; r.Cw = d->Cw;
    if (slice4) { r.slice4 = 1; r.Ktot = d->kT * d->kH * 32; }      // thin3 stems: 4-chunk slices, the 4th is no tap
    r.out_scale = out_scale; r.accumulate = zero_first ? 0 : 1;
    const int64_t total = (int64_t)r.Co * r.Kpad / 4;
    r.lanes = 1;
    while (r.lanes < 32 && r.lanes * 4 <= r.splits) r.lanes *= 2;
    hipLaunchKernelGGL(sf_wgrad_reduce_kernel, dim3(cdiv(total, SF_THREADS / r.lanes)), dim3(SF_THREADS), 0, s, r);
}

// One plan per weight gradient: the path that runs with its tiles, splits, padded extents and workspace.  Every path cuts the
// reduction over the M = N*To*Ho*Wo positions into splits; each stores fp32 partial tile sets ("slabs" of [Co_pad][Kpad]) with
// plain stores and sf_wgrad_reduce_kernel sums them (deterministic, no atomics).
enum WgradPath { WGRAD_GEN1, WGRAD_ROWTAB, WGRAD_STEM };
struct WgradPlan {
    WgradPath path;
    bool thin, dual;                    // WGRAD_ROWTAB: sf_wgrad2t_kernel / two splits per workgroup; neither: one split per workgroup
    int BMW, BKW, KS, tiles_k, tiles_c, Co_pad, Kpad;
    int nchunks, chunks_per_split;      // WGRAD_GEN1: 32-position chunks
    int rows_per_split, splits;         // (rows: WGRAD_ROWTAB)
    int slabs;                          // fp32 partial tile sets written (= splits, or split PAIRS of the dual kernel)
    size_t tab_bytes, ws_bytes;         // row table at the head of the workspace (WGRAD_ROWTAB); everything
    StemPlan stem;                      // plan_stem(d), evaluated once (WGRAD_STEM launches from it)
};
// WGRAD_GEN1 (sf_wgrad_kernel): ~4 workgroups per CU in flight
static WgradPlan plan_wgrad1(const sf_conv_desc* d) {
    WgradPlan w;
    memset(&w, 0, sizeof(w));
    w.path = WGRAD_GEN1;
    const int taps = d->kT * d->kH * d->kW;
    const int Ktot = taps * d->Ci;
    const int64_t M = (int64_t)d->N * d->To * d->Ho * d->Wo;
    w.BMW = wgrad1_bmw(d->Co); w.KS = wgrad1_ks(w.BMW);
    w.tiles_k = cdiv(Ktot, 128);
    w.tiles_c = cdiv(d->Co, w.BMW);
    w.Kpad = w.tiles_k * 128;
    w.Co_pad = w.tiles_c * w.BMW;
    w.nchunks = cdiv(M, 32);
    const int64_t slab = (int64_t)w.Co_pad * w.Kpad * 4;
    static const int target = tune_knob("SF_WGRAD_BLOCKS", 1024);
    int splits = cdiv(target, (int64_t)w.tiles_k * w.tiles_c);
    const int64_t cap = (256ll << 20) / slab;            // keep the workspace <= 256 MiB
    if (splits > cap) splits = (int)(cap < 1 ? 1 : cap);
    const int nstages = cdiv(w.nchunks, w.KS);
    if (splits > nstages) splits = nstages;
    if (splits < 1) splits = 1;
    w.chunks_per_split = cdiv(nstages, splits) * w.KS;   // whole stages per split
    w.splits = cdiv(w.nchunks, w.chunks_per_split);
    w.slabs = w.splits;
    w.ws_bytes = (size_t)slab * w.splits;
    return w;
}

// WGRAD_ROWTAB, the second-generation weight gradient (sf_wgrad2.h): plain (already activated) input, no stem, at least 33 output
// channels, a K axis that fills most of a 256-wide tile.  SF_WGRAD2=0 keeps the first kernel.  False: w is untouched.
static bool plan_wgrad2(const sf_conv_desc* d, WgradPlan& w) {
    if (test_hook("SF_WGRAD2", 1) == 0) return false;
    const int mink = test_hook("SF_WGRAD2_MINK", 192);
    const int minrows = test_hook("SF_WGRAD2_MINROWS", 4096);
    const int taps = d->kT * d->kH * d->kW;
    // Workgroups to aim for: ONE resident round (2 per CU x 256 CUs).  The split count is rounded DOWN so that the grid never
    // exceeds the target by a few workgroups: 18 tiles x 29 splits = 522 on 512 resident slots ran a second, almost empty round
    // (s4.slow b: 120 us at 522 workgroups, 99 us at 396; profiles/r3/r3_v2_wgrad_sweep.md -- which also records a one-workgroup-
    // per-CU six-stage ring with half the splits losing on every layer; that variant is gone again, commit 4267b0c has it).
    const int target = test_hook("SF_WGRAD2_BLOCKS", 512);
    const int Ktot = taps * d->Ci;
    const int64_t M = (int64_t)d->N * d->To * d->Ho * d->Wo;
    if (taps > SF_I2_MAXTAPS || M < minrows) return false;
    if ((d->kT - 1) * d->dT > 127 || (d->kH - 1) * d->dH > 127 || (d->kW - 1) * d->dW > 127) return false;
    if (d->Co <= 32) {
        // thin layers (sf_wgrad2t_kernel): one workgroup tile holds every output channel; SF_WGRAD2T=0 keeps the first kernel
        if (test_hook("SF_WGRAD2T", 1) == 0) return false;
        const int minrows_t = test_hook("SF_WGRAD2T_MINROWS", 16384);
        if (M < minrows_t) return false;
        w.thin = true;
        w.BMW = d->Co <= 16 ? 16 : 32;
        w.BKW = Ktot <= 32 ? 32 : 128;
        w.tiles_k = cdiv(Ktot, w.BKW);
        w.tiles_c = 1;
        w.Kpad = w.tiles_k * w.BKW;
        w.Co_pad = w.BMW;
        // one resident round of workgroups: LDS allows 2 per CU with 128-wide tiles (2 x 37-41 KB stages), 3 (BMW 32) or 4 (BMW 16)
        // with 32-wide ones; measured per layer, 512 / 768 / 1024 / 1536 / 2048: profiles/r2/r2_v24_wgrad_thin.md
        const int target_t = test_hook("SF_WGRAD2T_BLOCKS", w.BKW == 128 ? 512 : w.BMW == 32 ? 768 : 1024);
        int splits = target_t / w.tiles_k;                  // rounded down: never a few workgroups beyond the resident round
        if (splits < 1) splits = 1;
        w.rows_per_split = roundup(cdiv(M, splits), 128);
        w.splits = cdiv(M, w.rows_per_split);
        w.tab_bytes = ((size_t)M * 8 + 255) / 256 * 256 + 1280;  // pad: the thin kernel reads whole 32-byte groups up to one 128-position stage past M
        w.ws_bytes = w.tab_bytes + (size_t)w.Co_pad * w.Kpad * 4 * w.splits;
        w.slabs = w.splits;
        w.path = WGRAD_ROWTAB;
        return true;
    }
    if (Ktot < mink) return false;
    w.BMW = d->Co > 64 ? 128 : 64;       // 64-row co-tiles for wide layers lose 20-40 % on res3-res5 (profiles/r3/r3_final_wgrad_sweep.md)
    w.tiles_k = cdiv(Ktot, 256);
    w.tiles_c = cdiv(d->Co, w.BMW);
    w.Kpad = w.tiles_k * 256;
    w.Co_pad = w.tiles_c * w.BMW;
    int splits = target / (w.tiles_k * w.tiles_c);
    const int64_t slab = (int64_t)w.Co_pad * w.Kpad * 4;
    const int64_t cap = (256ll << 20) / slab;
    if (splits > cap) splits = (int)(cap < 1 ? 1 : cap);
    if (splits < 1) splits = 1;
    // two splits per 1024-thread workgroup, summed through LDS before anything is stored (sf_wgrad2_kernel<., true>): the same
    // waves, rings and position ranges per CU, half the partial tiles.  The resident round is then target / 2 workgroups of
    // PAIRS: the pair count is rounded down against it (24 tiles x 11 pairs = 264 workgroups on 256 CUs ran a second round:
    // 110 -> 191 us, profiles/r6_v15_wgrad_sweep_dual.md).  SF_WGRAD2_DUAL=0 keeps one split per workgroup.
    // Taken where it pays (per layer, profiles/r6_v16_wgrad_sweep_dual.md): short position loops (many splits of few steps: the
    // stores and the reduction are a large share -- s4 c 256 -> 1024 57 -> 49 us, s3 a 512 -> 128 87 -> 56 us), not the long
    // loops of the 3x1x1 layers (the shared barrier costs them ~3 %), and only when the pairs fill the chip as well as the
    // single splits did (96 tiles: 2 pairs = 192 workgroups against 5 splits = 480 halves: 117 -> 133 us).
    w.dual = false;
    if (splits >= 2 && test_hook("SF_WGRAD2_DUAL", 1) != 0) {
        const int tiles = w.tiles_k * w.tiles_c;
        const int pairs = (target / 2) / tiles;
        const int64_t steps = cdiv(cdiv(M, splits), 32);
        if (pairs >= 1 && 2 * pairs * 10 >= (2 * pairs < splits ? splits : 2 * pairs) * 9 && steps <= test_hook("SF_WGRAD2_DUAL_STEPS", 80)) {
            w.dual = true;
            if (2 * pairs < splits) splits = 2 * pairs;
        }
    }
    w.rows_per_split = roundup(cdiv(M, splits), 32);
    w.splits = cdiv(M, w.rows_per_split);
    if (w.splits < 2) w.dual = false;
    w.slabs = w.dual ? cdiv(w.splits, 2) : w.splits;
    w.tab_bytes = ((size_t)M * 8 + 255) / 256 * 256 + 1280;  // pad: the thin kernel reads whole 32-byte groups up to one 128-position stage past M
    w.ws_bytes = w.tab_bytes + (size_t)slab * w.splits;
    w.path = WGRAD_ROWTAB;
    return true;
}
// The path sf_conv_wgrad takes: the row-table kernel, else the direct-convolution stem kernel (both read a plain input: a fused
// input BatchNorm, `in_affine`, keeps the first generation), else the first generation.
static WgradPlan plan_conv_wgrad(const sf_conv_desc* d, bool in_affine) {
    const StemPlan sp = plan_stem(d);
    WgradPlan w;
    memset(&w, 0, sizeof(w));
    if (in_affine || !(sp.ok || plan_wgrad2(d, w))) w = plan_wgrad1(d);
    else if (sp.ok) {
        w.path = WGRAD_STEM;
        w.slabs = sp.wg_blocks * sp.wgroups; w.Co_pad = 16; w.Kpad = sp.Kpad; w.ws_bytes = sp.ws_bytes;
    }
    w.stem = sp;
    return w;
}

// Row table of the v2 weight-gradient kernel ({first input position, tap-validity mask} per output row): a function of the
// convolution geometry alone, so a caller may build it once (sf_conv_wgrad_rowtab) and pass it to every sf_conv_wgrad call.
static void launch_rowtab(const sf_conv_desc* d, void* tab, hipStream_t s) {
    RowtabParams t;
    memset(&t, 0, sizeof(t));
    t.tab = (i32x2*)tab;
    t.M = d->N * d->To * d->Ho * d->Wo;
    t.fdW = make_fastdiv(d->Wo); t.fdH = make_fastdiv(d->Ho); t.fdT = make_fastdiv(d->To);
    t.sT = d->Ti; t.sH = d->Hi; t.sW = d->Wi;
    t.strT = d->sT; t.strH = d->sH; t.strW = d->sW; t.padT = d->pT; t.padH = d->pH; t.padW = d->pW;
    t.ntaps = d->kT * d->kH * d->kW;
    int ti = 0;
    for (int kt = 0; kt < d->kT; ++kt)
        for (int kh = 0; kh < d->kH; ++kh)
            for (int kw = 0; kw < d->kW; ++kw, ++ti) {
                t.dt[ti] = (int8_t)(kt * d->dT); t.dh[ti] = (int8_t)(kh * d->dH); t.dw[ti] = (int8_t)(kw * d->dW);
            }
    hipLaunchKernelGGL(sf_wgrad2_rowtab_kernel, dim3(cdiv(t.M, SF_THREADS)), dim3(SF_THREADS), 0, s, t);
}

extern "C" int64_t sf_conv_wgrad_rowtab_bytes(const sf_conv_desc* d) {
    if (check_desc(d)) return -1;
    return (int64_t)plan_conv_wgrad(d, false).tab_bytes;
}

extern "C" int sf_conv_wgrad_rowtab(const sf_conv_desc* d, void* tab, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(tab && (uintptr_t)tab % 16 == 0, "sf_conv_wgrad_rowtab: tab must be a 16-byte aligned device pointer");
    REQUIRE(plan_conv_wgrad(d, false).path == WGRAD_ROWTAB, "sf_conv_wgrad_rowtab: this geometry does not take the row-table kernel (sf_conv_wgrad_rowtab_bytes == 0)");
    launch_rowtab(d, tab, (hipStream_t)stream);
    return check_launch("wgrad_rowtab");
}

extern "C" int64_t sf_conv_wgrad_workspace(const sf_conv_desc* d) {
    if (check_desc(d)) return -1;
    // the larger of the two paths the geometry can take: callers keep one value per geometry, with or without a fused input BatchNorm
    const int64_t plain = (int64_t)plan_conv_wgrad(d, false).ws_bytes, affine = (int64_t)plan_conv_wgrad(d, true).ws_bytes;
    return plain > affine ? plain : affine;
}

// The partial tile sets of a planned weight gradient: `slabs` receives w.slabs sets of [Co_pad][Kpad] floats; `tab` is the row
// table of the WGRAD_ROWTAB kernels (already built), `workspace` the head of the caller's workspace (WGRAD_STEM writes there).
// `bundles` > 0 (sf_gconv_wgrad): d is the geometry of ONE bundle of d->Ci channels, x / dy / slabs those of bundle 0; the BUNDLED
// kernels take bundle blockIdx.y from the same rows, d->Ci channels and one slab set further on.
static void launch_wgrad_partials(const sf_conv_desc* d, const WgradPlan& w, const GatherSide& gk, const void* x, const void* dy,
                                  float* slabs, const void* tab, void* workspace, hipStream_t s, int bundles = 0) {
    if (w.path == WGRAD_ROWTAB) {
        Wgrad2Params q;
        memset(&q, 0, sizeof(q));
        int ti = 0;
        for (int kt = 0; kt < d->kT; ++kt)
            for (int kh = 0; kh < d->kH; ++kh)
                for (int kw = 0; kw < d->kW; ++kw, ++ti) q.dlin[ti] = (kt * d->dT * d->Hi + kh * d->dH) * d->Wi + kw * d->dW;
        q.x = (const f16*)x; q.ldx = d->ldx; q.C = d->Ci;
        q.dy = (const f16*)dy; q.ldy = d->ldy; q.Co = d->Co;
        q.M = d->N * d->To * d->Ho * d->Wo; q.Ktot = gk.Ktot;
        q.rowtab = (const i32x2*)tab;
        q.ws = slabs; q.Co_pad = w.Co_pad; q.Kpad = w.Kpad;
        q.tiles_k = w.tiles_k; q.tiles_c = w.tiles_c; q.rows_per_split = w.rows_per_split;
        q.stage_stride = (w.thin && tune_knob("SF_WGRAD2T_RR", 1) != 0) ? w.splits : 0;
        const dim3 grid((unsigned)(w.tiles_k * w.tiles_c * w.slabs), bundles > 0 ? (unsigned)bundles : 1u);
        if (sf_trace()) fprintf(stderr, "[sfamd] wgrad2: M=%d Co=%d K=%d tiles %dx%d splits %d%s\n", q.M, q.Co, q.Ktot, w.tiles_c, w.tiles_k, w.splits,
                                w.dual ? " (two per workgroup)" : "");
        if (bundles > 0) {          // 32- and 64-channel bundles: the thin 32 x 128 tile, the 64-row tile with one split per workgroup
            if (w.thin) hipLaunchKernelGGL((sf_wgrad2t_kernel<32, 128, 2, true>), grid, dim3(256), 0, s, q);
            else hipLaunchKernelGGL((sf_wgrad2_kernel<64, false, true>), grid, dim3(512), 0, s, q);
        } else if (w.thin) {
            if (w.BMW == 16 && w.BKW == 128) hipLaunchKernelGGL((sf_wgrad2t_kernel<16, 128, 2>), grid, dim3(256), 0, s, q);
            else if (w.BMW == 32 && w.BKW == 128) hipLaunchKernelGGL((sf_wgrad2t_kernel<32, 128, 2>), grid, dim3(256), 0, s, q);
            else if (w.BMW == 16) hipLaunchKernelGGL((sf_wgrad2t_kernel<16, 32, 3>), grid, dim3(256), 0, s, q);
            else hipLaunchKernelGGL((sf_wgrad2t_kernel<32, 32, 3>), grid, dim3(256), 0, s, q);
        } else if (w.dual) {
            if (w.BMW == 128) hipLaunchKernelGGL((sf_wgrad2_kernel<128, true>), grid, dim3(1024), 0, s, q);
            else hipLaunchKernelGGL((sf_wgrad2_kernel<64, true>), grid, dim3(1024), 0, s, q);
        } else {
            if (w.BMW == 128) hipLaunchKernelGGL((sf_wgrad2_kernel<128>), grid, dim3(512), 0, s, q);
            else hipLaunchKernelGGL((sf_wgrad2_kernel<64>), grid, dim3(512), 0, s, q);
        }
    } else if (w.path == WGRAD_STEM) {
        const StemPlan& sp = w.stem;
        StemParams q = stem_params(d, sp, x);
        q.dy = (const f16*)dy; q.ws = (float*)workspace;
        if (sf_trace()) fprintf(stderr, "[sfamd] stem_wgrad: %d workgroups x %d tiles\n", sp.wg_blocks, sp.tiles_per_block);
        static const bool stem_plain = tune_knob("SF_STEM_XCD", 1) == 0;
        q.plain_order = stem_plain ? 1 : 0;
        const dim3 grid(sp.wg_blocks), block(SF_STEM_WG_THREADS);
        if (d->Co <= 8 && sp.small) hipLaunchKernelGGL((sf_stem_wgrad_kernel<8, SF_STEM_CHUNKS_SMALL>), grid, block, 0, s, q);
        else if (d->Co <= 8) hipLaunchKernelGGL((sf_stem_wgrad_kernel<8, SF_STEM_CHUNKS>), grid, block, 0, s, q);
        else if (sp.small) hipLaunchKernelGGL((sf_stem_wgrad_kernel<16, SF_STEM_CHUNKS_SMALL>), grid, block, 0, s, q);
        else hipLaunchKernelGGL((sf_stem_wgrad_kernel<16, SF_STEM_CHUNKS>), grid, block, 0, s, q);
    } else {
        WgradParams p;
        memset(&p, 0, sizeof(p));
        p.g = gk;
        p.dy = (const f16*)dy; p.ldy = d->ldy; p.Co = d->Co;
        p.M = d->N * d->To * d->Ho * d->Wo;
        p.ws = slabs; p.Co_pad = w.Co_pad; p.Kpad = w.Kpad;
        p.nchunks = w.nchunks; p.chunks_per_split = w.chunks_per_split;
        if (bundles > 0) {
            p.tiles_k = w.tiles_k; p.tiles_c = w.tiles_c;
            const dim3 grid((unsigned)(w.tiles_k * w.tiles_c * w.splits), (unsigned)bundles), block(SF_THREADS);
            if (w.BMW == 64) hipLaunchKernelGGL((sf_wgrad_kernel<64, 32, 64, 1, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((sf_wgrad_kernel<32, 32, 32, 4, true>), grid, block, 0, s, p);
            return;
        }
        launch_wgrad1(w.BMW, p, dim3(w.tiles_k, w.tiles_c, w.splits), s);
    }
}

extern "C" int sf_conv_wgrad(const sf_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                             int in_relu, const void* dy, float* dw, float out_scale, int zero_first,
                             void* workspace, int64_t workspace_bytes, const void* rowtab, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(x && dy && dw && workspace, "sf_conv_wgrad: null pointer");
    REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "sf_conv_wgrad: in_scale/in_shift must come together");
    REQUIRE(!in_scale || d->Ci <= 512, "sf_conv_wgrad: fused input BatchNorm supports Ci <= 512 (got %d)", d->Ci);
    hipStream_t s = (hipStream_t)stream;
    GatherSide gk = gather_fwd(d, x, in_scale, in_shift, in_relu);
    const WgradPlan w = plan_conv_wgrad(d, in_scale != nullptr);
    REQUIRE(workspace_bytes >= (int64_t)w.ws_bytes, "sf_conv_wgrad: workspace too small (%lld < %lld bytes)",
            (long long)workspace_bytes, (long long)w.ws_bytes);
    float* slabs = (float*)((char*)workspace + w.tab_bytes);
    if (w.path == WGRAD_ROWTAB) {
        REQUIRE(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)workspace) % 16 == 0, "sf_conv_wgrad: operands must be 16-byte aligned");
        if (!rowtab) launch_rowtab(d, workspace, s);     // the caller keeps no table for this geometry: build it per call
        else REQUIRE((uintptr_t)rowtab % 16 == 0, "sf_conv_wgrad: rowtab must be 16-byte aligned");
    } else if (w.path == WGRAD_GEN1) {
        REQUIRE(w.splits <= 65535, "sf_conv_wgrad: too many splits");
    }
    launch_wgrad_partials(d, w, gk, x, dy, slabs, rowtab ? rowtab : workspace, workspace, s);
    if (check_launch("wgrad")) return -1;
    launch_wgrad_reduce(d, slabs, w.slabs, w.Co_pad, w.Kpad, w.path == WGRAD_STEM && w.stem.thin3, dw, out_scale, zero_first, s);
    return check_launch("wgrad_reduce");
}

// ------------------------------------------------------------------------------------------------
// Grouped 1x3x3 convolution on block-diagonal tiles (sf_gconv.h; resnet_helper.py:346-358 with groups = num_groups).  d->Ci == d->Co
// is the channel count C of the activation, d->Cw the channels per group Cg of the fp32 weight [C][Cg][1][3][3].
static inline int gconv_bundle(const sf_conv_desc* d) { return d->Cw > 32 ? d->Cw : 32; }
static int check_gconv(const char* who, const sf_conv_desc* d) {
    if (check_desc(d)) return -1;
    REQUIRE(d->kT == 1 && d->kH == 3 && d->kW == 3, "%s: kernel (%d,%d,%d) is not supported: grouped convolutions are (1,3,3)", who,
            d->kT, d->kH, d->kW);
    REQUIRE(d->Ci == d->Co && (d->Cow == 0 || d->Cow == d->Co), "%s: a grouped convolution maps C to C channels (Ci=%d Co=%d Cow=%d)",
            who, d->Ci, d->Co, d->Cow);
    const int Cg = d->Cw;
    REQUIRE(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64,
            "%s: %d channels per group are not supported: Cg must be one of 4, 8, 16, 32, 64", who, Cg);
    const int B = gconv_bundle(d);
    REQUIRE(d->Ci % B == 0, "%s: C=%d with Cg=%d is not a whole number of %d-channel bundles", who, d->Ci, Cg, B);
    REQUIRE(d->sT == 1 && d->sH == d->sW && (d->sH == 1 || d->sH == 2), "%s: stride (%d,%d,%d) is not supported: (1,1,1) or (1,2,2)",
            who, d->sT, d->sH, d->sW);
    REQUIRE(d->dT == 1 && d->dH == d->dW && (d->dH == 1 || d->dH == 2) && d->pT == 0 && d->pH == d->dH && d->pW == d->dW,
            "%s: dilation (%d,%d,%d) / padding (%d,%d,%d) is not supported: dilation (1,k,k) with k = 1 or 2 and padding (0,k,k)", who,
            d->dT, d->dH, d->dW, d->pT, d->pH, d->pW);
    return 0;
}
// the descriptor of one bundle: the dense B -> B convolution on the pitched rows of the whole tensor
static sf_conv_desc gconv_bundle_desc(const sf_conv_desc* d) {
    sf_conv_desc b = *d;
    b.Ci = b.Co = b.Cw = gconv_bundle(d);
    b.Cow = 0;
    return b;
}
// sf_igemm2_kernel<.., BUNDLED>: 256 x 32 x 32 tiles for the 32-wide bundles, 256 x 64 tiles for the 64-wide ones (64 deep when the
// grid is at most ~one tile per CU: plan_gemm2_tile's rule).  The tap columns of the mirrored data-gradient operand: `mirror`.
static void gconv_launch(Igemm2Params& q, const sf_conv_desc* d, bool mirror, hipStream_t s) {
    const int B = gconv_bundle(d), nb = d->Ci / B;
    q.bundle_w = B; q.stat_ld = d->Co;
    if (mirror)
        for (int t = 0; t < q.ntaps; ++t) q.taps[t].wcol = (9 - 1) * B - q.taps[t].wcol;
    const int mtiles = cdiv(q.M, 256);
    q.ntiles_n = 1;
    const dim3 grid((unsigned)mtiles, (unsigned)nb), block(512);
    if (sf_trace()) fprintf(stderr, "[sfamd] gconv igemm2: M=%d bundles %d x %d taps=%d omap=%d\n", q.M, nb, B, q.ntaps, q.omap);
    if (B == 32) hipLaunchKernelGGL((sf_igemm2_kernel<256, 32, 4, 2, 32, 3, false, true>), grid, block, 0, s, q);
    else if ((int64_t)mtiles * nb <= 320) hipLaunchKernelGGL((sf_igemm2_kernel<256, 64, 4, 2, 64, 3, false, true>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((sf_igemm2_kernel<256, 64, 4, 2, 32, 3, false, true>), grid, block, 0, s, q);
}
static int check_gconv_act(const char* who, const void* a, int ld, int C) {
    REQUIRE(a && (uintptr_t)a % 16 == 0 && ld >= C && ld % 8 == 0, "%s: activations must be 16-byte aligned with a pitch % 8 == 0 >= C", who);
    return 0;
}

extern "C" int sf_gconv_prep_weights(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_stream_t stream) {
    if (check_gconv("sf_gconv_prep_weights", d)) return -1;
    REQUIRE(w && wf, "sf_gconv_prep_weights: null pointer");
    GconvPrepParams p;
    memset(&p, 0, sizeof(p));
    p.w = w; p.wf = (f16*)wf; p.wd = (f16*)wd; p.C = d->Co; p.Cg = d->Cw; p.B = gconv_bundle(d); p.taps = 9;
    const int64_t total = (int64_t)p.C * p.taps * p.B * (wd ? 2 : 1);
    int blocks = cdiv(total, SF_THREADS);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sf_gconv_prep_kernel, dim3(blocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("gconv_prep_weights");
}

extern "C" int sf_gconv_fwd(const sf_conv_desc* d, const void* x, const void* wf, const float* bias, int out_relu, void* y,
                            float* stat_part, sf_stream_t stream) {
    if (check_gconv("sf_gconv_fwd", d)) return -1;
    REQUIRE(wf && (uintptr_t)wf % 16 == 0, "sf_gconv_fwd: the packed weight must be 16-byte aligned");
    if (check_gconv_act("sf_gconv_fwd", x, d->ldx, d->Ci) || check_gconv_act("sf_gconv_fwd", y, d->ldy, d->Co)) return -1;
    const sf_conv_desc b = gconv_bundle_desc(d);
    IgemmParams p = gemm_params(gather_fwd(&b, x, nullptr, nullptr, 0), d->N * d->To * d->Ho * d->Wo, wf, 9 * b.Ci, b.Co, y, d->ldy,
                                bias, nullptr, 0);
    p.stat_part = stat_part;
    p.act_mode = out_relu ? 3 : 0;
    Igemm2Params q;
    igemm2_dense(q, p);
    gconv_launch(q, d, false, (hipStream_t)stream);
    return check_launch("gconv_fwd");
}

extern "C" int sf_gconv_dgrad(const sf_conv_desc* d, const void* dy, const void* wd, void* dx, sf_stream_t stream) {
    if (check_gconv("sf_gconv_dgrad", d)) return -1;
    REQUIRE(wd && (uintptr_t)wd % 16 == 0, "sf_gconv_dgrad: the packed weight must be 16-byte aligned");
    if (check_gconv_act("sf_gconv_dgrad", dy, d->ldy, d->Co) || check_gconv_act("sf_gconv_dgrad", dx, d->ldx, d->Ci)) return -1;
    const sf_conv_desc b = gconv_bundle_desc(d);
    IgemmParams p = gemm_params(gather_dgrad(&b, dy), d->N * d->Ti * d->Hi * d->Wi, wd, 9 * b.Co, b.Ci, dx, d->ldx, nullptr, nullptr, 0);
    Igemm2Params q;
    if (d->sH == 1) {
        igemm2_dense(q, p);
        gconv_launch(q, d, true, (hipStream_t)stream);
    } else {            // one launch per stride-residue class of input positions (igemm2_class), every bundle in each
        for (int rh = 0; rh < d->sH; ++rh)
            for (int rw = 0; rw < d->sW; ++rw) {
                const int r[3] = {0, rh, rw};
                if (!igemm2_class(q, p, r)) continue;
                gconv_launch(q, d, true, (hipStream_t)stream);
            }
    }
    return check_launch("gconv_dgrad");
}

// The bundles share ONE grid (blockIdx.y of the BUNDLED weight-gradient kernels): the dense planner picks the path and the tiles for
// the B -> B geometry of a bundle, and each bundle takes 1 / nb of the splits that plan gives a whole layer -- together they fill
// the chip once, as one dense layer does.  One split per workgroup (the pair kernel is not used).  Workspace: the row table, then
// nb sets of `slabs` partial tiles.
static WgradPlan plan_gconv_wgrad(const sf_conv_desc* b, int nb) {
    WgradPlan w = plan_conv_wgrad(b, false);
    const int64_t M = (int64_t)b->N * b->To * b->Ho * b->Wo;
    int splits = w.splits / nb;
    if (splits < 1) splits = 1;
    if (w.path == WGRAD_ROWTAB) {
        w.dual = false;
        w.rows_per_split = roundup(cdiv(M, splits), w.thin ? 128 : 32);
        w.splits = cdiv(M, w.rows_per_split);
    } else if (w.path == WGRAD_GEN1) {
        const int nstages = cdiv(w.nchunks, w.KS);
        if (splits > nstages) splits = nstages;
        w.chunks_per_split = cdiv(nstages, splits) * w.KS;
        w.splits = cdiv(w.nchunks, w.chunks_per_split);
    }
    w.slabs = w.splits;
    w.ws_bytes = w.tab_bytes + (size_t)nb * w.slabs * w.Co_pad * w.Kpad * 4;
    return w;
}

extern "C" int64_t sf_gconv_wgrad_workspace(const sf_conv_desc* d) {
    if (check_gconv("sf_gconv_wgrad_workspace", d)) return -1;
    const sf_conv_desc b = gconv_bundle_desc(d);
    return (int64_t)plan_gconv_wgrad(&b, d->Ci / b.Ci).ws_bytes;
}

extern "C" int sf_gconv_wgrad(const sf_conv_desc* d, const void* x, const void* dy, float* dw, float out_scale, int zero_first,
                              void* workspace, int64_t workspace_bytes, sf_stream_t stream) {
    if (check_gconv("sf_gconv_wgrad", d)) return -1;
    REQUIRE(dw && workspace && (uintptr_t)workspace % 16 == 0, "sf_gconv_wgrad: null or unaligned pointer");
    if (check_gconv_act("sf_gconv_wgrad", x, d->ldx, d->Ci) || check_gconv_act("sf_gconv_wgrad", dy, d->ldy, d->Co)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const sf_conv_desc b = gconv_bundle_desc(d);
    const int B = b.Ci, nb = d->Ci / B, Cg = d->Cw;
    const WgradPlan w = plan_gconv_wgrad(&b, nb);
    REQUIRE(w.path != WGRAD_STEM && w.BMW == B && (w.path != WGRAD_ROWTAB || !w.thin || w.BKW == 128), "sf_gconv_wgrad: unexpected plan");
    REQUIRE(workspace_bytes >= (int64_t)w.ws_bytes, "sf_gconv_wgrad: workspace too small (%lld < %lld bytes)",
            (long long)workspace_bytes, (long long)w.ws_bytes);
    REQUIRE(nb <= 65535, "sf_gconv_wgrad: too many bundles");
    float* slabs = (float*)((char*)workspace + w.tab_bytes);
    if (w.path == WGRAD_ROWTAB) launch_rowtab(&b, workspace, s);
    const GatherSide gk = gather_fwd(&b, x, nullptr, nullptr, 0);
    launch_wgrad_partials(&b, w, gk, x, dy, slabs, workspace, workspace, s, nb);
    if (check_launch("gconv_wgrad")) return -1;
    GconvReduceParams r;
    memset(&r, 0, sizeof(r));
    r.ws = slabs; r.slabs = w.slabs; r.Co_pad = w.Co_pad; r.Kpad = w.Kpad; r.bundle_ws = (int64_t)w.slabs * w.Co_pad * w.Kpad;
    r.dw = dw; r.C = d->Co; r.Cg = Cg; r.B = B; r.taps = 9;
    r.out_scale = out_scale; r.accumulate = zero_first ? 0 : 1;
    hipLaunchKernelGGL(sf_gconv_wgrad_reduce_kernel, dim3(cdiv((int64_t)d->Co * Cg * 9, SF_THREADS)), dim3(SF_THREADS), 0, s, r);
    return check_launch("gconv_wgrad_reduce");
}

// ------------------------------------------------------------------------------------------------
// Block-final BatchNorm backward + both gradients of conv c in one persistent launch (sf_cbwd.h).  ONE planner decides who takes it:
// 1x1x1, unit stride, unpadded, Ci % 8 == 0 <= 64, Co % 32 == 0 <= 256, a plain (already activated) input and the bit-mask form of
// the block-output ReLU -- never the row count, so that small test models take the production path.  SF_CBWD=0 (test hook) keeps the
// three launches; SF_CBWD_WGS (test hook) sets the workgroup count so that a small tensor makes every workgroup walk several tiles.
// The rows are dealt to the workgroups exactly as sf_conv_wgrad deals them to its splits (plan_wgrad1: contiguous runs of 32-row
// chunks; plan_wgrad2's thin kernel: 128-row stages round robin, the four waves a quarter each), every 32-row MFMA step lands on the
// accumulator it lands on there and the slabs meet in the same sf_wgrad_reduce_kernel launch: dw has the bits of the three-launch
// path.  The inner BatchNorm's table keeps the 128-row tiles and the per-thread order of the data gradient's epilogue.
struct CbwdPlan {
    bool ok;
    int cip, cop, R;
    size_t ws_bytes;
};
#define SF_CBWD_MAX_WGS 1024
template <int CIP, int COP>
static void cbwd_fill(CbwdPlan& w) {
    using K = CbwdCfg<CIP, COP>;
    w.R = K::R;
    w.ws_bytes = (size_t)SF_CBWD_MAX_WGS * COP * CIP * 4;
}
#define SF_CBWD_FOR_SHAPE(cip, cop, ...)                                                         \
    do {                                                                                         \
        if ((cip) == 16 && (cop) == 32) { constexpr int CIP_ = 16, COP_ = 32; __VA_ARGS__; }            \
        else if ((cip) == 16 && (cop) == 64) { constexpr int CIP_ = 16, COP_ = 64; __VA_ARGS__; }       \
        else if ((cip) == 16 && (cop) == 128) { constexpr int CIP_ = 16, COP_ = 128; __VA_ARGS__; }     \
        else if ((cip) == 16 && (cop) == 256) { constexpr int CIP_ = 16, COP_ = 256; __VA_ARGS__; }     \
        else if ((cip) == 32 && (cop) == 32) { constexpr int CIP_ = 32, COP_ = 32; __VA_ARGS__; }       \
        else if ((cip) == 32 && (cop) == 64) { constexpr int CIP_ = 32, COP_ = 64; __VA_ARGS__; }       \
        else if ((cip) == 32 && (cop) == 128) { constexpr int CIP_ = 32, COP_ = 128; __VA_ARGS__; }     \
        else if ((cip) == 32 && (cop) == 256) { constexpr int CIP_ = 32, COP_ = 256; __VA_ARGS__; }     \
        else if ((cip) == 64 && (cop) == 32) { constexpr int CIP_ = 64, COP_ = 32; __VA_ARGS__; }       \
        else if ((cip) == 64 && (cop) == 64) { constexpr int CIP_ = 64, COP_ = 64; __VA_ARGS__; }       \
        else if ((cip) == 64 && (cop) == 128) { constexpr int CIP_ = 64, COP_ = 128; __VA_ARGS__; }     \
        else if ((cip) == 64 && (cop) == 256) { constexpr int CIP_ = 64, COP_ = 256; __VA_ARGS__; }     \
        else if ((cip) == 128 && (cop) == 32) { constexpr int CIP_ = 128, COP_ = 32; __VA_ARGS__; }     \
        else if ((cip) == 128 && (cop) == 64) { constexpr int CIP_ = 128, COP_ = 64; __VA_ARGS__; }     \
        else if ((cip) == 128 && (cop) == 128) { constexpr int CIP_ = 128, COP_ = 128; __VA_ARGS__; }   \
        else { constexpr int CIP_ = 128, COP_ = 256; __VA_ARGS__; }                                     \
    } while (0)
// Who sums which of the M output rows: as the weight gradient of the three-launch path would (see above).  Returns the workgroup
// count; *rps = rows per workgroup, or 0 for the round robin over 128-row tiles of the thin plan.
static int cbwd_deal_rows(const sf_conv_desc* d, int64_t M, int* rps) {
    const WgradPlan w2 = plan_conv_wgrad(d, false);
    const int forced = test_hook("SF_CBWD_WGS", 0);
    if (forced > 0) {
        const int wgs = forced < SF_CBWD_MAX_WGS ? forced : SF_CBWD_MAX_WGS;
        *rps = roundup(cdiv(M, wgs), 32);
        return cdiv(M, *rps);
    }
    if (w2.path == WGRAD_ROWTAB && w2.thin && w2.splits <= SF_CBWD_MAX_WGS) {
        *rps = 0;
        return w2.splits;
    }
    const WgradPlan w1 = plan_wgrad1(d);
    *rps = w1.chunks_per_split * 32;
    return w1.splits;
}
static CbwdPlan plan_cbwd(const sf_conv_desc* d, bool in_affine, bool mask_bits) {
    CbwdPlan w;
    memset(&w, 0, sizeof(w));
    if (test_hook("SF_CBWD", 1) == 0) return w;
    if (d->kT != 1 || d->kH != 1 || d->kW != 1 || d->sT != 1 || d->sH != 1 || d->sW != 1 || d->pT || d->pH || d->pW) return w;
    if (d->To != d->Ti || d->Ho != d->Hi || d->Wo != d->Wi) return w;
    if (d->Ci % 8 || d->Ci > 64 || d->Co % 32 || d->Co > 256) return w;
    if (in_affine || !mask_bits) return w;
    w.cip = d->Ci <= 16 ? 16 : d->Ci <= 32 ? 32 : 64;
    w.cop = d->Co <= 32 ? 32 : d->Co <= 64 ? 64 : d->Co <= 128 ? 128 : 256;
    SF_CBWD_FOR_SHAPE(w.cip, w.cop, (cbwd_fill<CIP_, COP_>(w)));
    w.ok = true;
    return w;
}

extern "C" int sf_conv_c_bwd_plan(const sf_conv_desc* d, int in_affine, int mask_bits, int32_t* tile_rows,
                                  int64_t* workspace_bytes) {
    if (check_desc(d)) return -1;
    const CbwdPlan w = plan_cbwd(d, in_affine != 0, mask_bits != 0);
    if (tile_rows) *tile_rows = w.ok ? 128 : 0;
    if (workspace_bytes) *workspace_bytes = w.ok ? (int64_t)w.ws_bytes : 0;
    return w.ok ? 1 : 0;
}

extern "C" int sf_conv_c_bwd(const sf_conv_desc* d, const void* dz, int32_t lddz, const void* mask_bits, const void* yc,
                             int32_t ldyc, const float* coef, const void* act, const void* wd, const float* bn_scale,
                             const float* bn_shift, const void* bn_y, int32_t bn_ldy, float* bn_part, int32_t bn_part_rows,
                             int32_t* bn_rows, void* d_in, int32_t ld_in, float* dw, float out_scale, int zero_first,
                             void* workspace, int64_t workspace_bytes, sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(dz && mask_bits && yc && coef && act && wd && d_in && dw && workspace, "sf_conv_c_bwd: null pointer");
    const CbwdPlan w = plan_cbwd(d, false, true);
    REQUIRE(w.ok, "sf_conv_c_bwd: this geometry keeps sf_bn_bwd_apply + sf_conv_wgrad + sf_conv_dgrad_bn (sf_conv_c_bwd_plan == 0)");
    REQUIRE(lddz >= d->Co && lddz % 8 == 0 && ldyc >= d->Co && ldyc % 8 == 0 && ld_in >= d->Ci && ld_in % 8 == 0,
            "sf_conv_c_bwd: bad row pitch");
    REQUIRE((((uintptr_t)dz | (uintptr_t)yc | (uintptr_t)act | (uintptr_t)wd | (uintptr_t)d_in | (uintptr_t)workspace) & 15) == 0,
            "sf_conv_c_bwd: operands must be 16-byte aligned");
    REQUIRE(workspace_bytes >= (int64_t)w.ws_bytes, "sf_conv_c_bwd: workspace too small (%lld < %lld bytes)",
            (long long)workspace_bytes, (long long)w.ws_bytes);
    const int64_t M = (int64_t)d->N * d->Ti * d->Hi * d->Wi;
    const int ntiles = cdiv(M, 128);
    const bool fuse = bn_part != nullptr;
    if (fuse) {
        REQUIRE(bn_scale && bn_shift && bn_y && bn_rows, "sf_conv_c_bwd: the fused reduction needs bn_scale, bn_shift, bn_y and bn_rows");
        REQUIRE(bn_ldy >= d->Ci && bn_ldy % 8 == 0 && ((uintptr_t)bn_y & 15) == 0, "sf_conv_c_bwd: bad bn_y pitch / alignment");
        REQUIRE(bn_part_rows >= ntiles, "sf_conv_c_bwd: the partial table needs ceil(positions / tile_rows) rows of [2][Ci] floats");
    }
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    CbwdParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.Ci = d->Ci; p.Co = d->Co;
    p.dz = (const f16*)dz; p.lddz = lddz; p.bits = (const uint8_t*)mask_bits; p.yc = (const f16*)yc; p.ldyc = ldyc;
    p.coef = coef; p.act = (const f16*)act; p.ldact = d->ldx; p.wd = (const f16*)wd; p.ldw = ldd;
    if (fuse) { p.bnb_y = (const f16*)bn_y; p.bnb_ld = bn_ldy; p.bnb_scale = bn_scale; p.bnb_shift = bn_shift; p.bnb_part = bn_part; }
    p.dx = (f16*)d_in; p.lddx = ld_in; p.ws = (float*)workspace; p.tiles128 = ntiles;
    const int wgs = cbwd_deal_rows(d, M, &p.rps);
    REQUIRE(wgs <= SF_CBWD_MAX_WGS, "sf_conv_c_bwd: %d splits", wgs);
    hipStream_t s = (hipStream_t)stream;
    SF_CBWD_FOR_SHAPE(w.cip, w.cop, hipLaunchKernelGGL((sf_cbwd_kernel<CIP_, COP_>), dim3(wgs), dim3(SF_THREADS), 0, s, p));
    if (check_launch("conv_c_bwd")) return -1;
    if (bn_rows) *bn_rows = fuse ? ntiles : 0;
    launch_wgrad_reduce(d, (const float*)workspace, wgs, w.cop, w.cip, false, dw, out_scale, zero_first, s);
    return check_launch("conv_c_bwd_reduce");
}

// The projection shortcut of a stage's first block (branch1 + branch1_bn): the same kernel with the block input in the place of
// act_b, no inner BatchNorm, Ci up to 128 and -- at a spatial stride of 2 -- the row map of sf_cbwd.h.  Its own planner (again the
// geometry alone; SF_CBWD=0 switches the whole family off): 1x1x1, unpadded, undilated, stride (1,1,1) or (1,2,2) over even H and W.
// The rows are OUTPUT rows, dealt as above; the workspace is one slab per workgroup of that deal.
static CbwdPlan plan_proj_bwd(const sf_conv_desc* d, bool in_affine, bool mask_bits) {
    CbwdPlan w;
    memset(&w, 0, sizeof(w));
    if (test_hook("SF_CBWD", 1) == 0) return w;
    if (d->kT != 1 || d->kH != 1 || d->kW != 1 || d->pT || d->pH || d->pW || d->dT != 1 || d->dH != 1 || d->dW != 1) return w;
    const bool unit = d->sH == 1 && d->sW == 1 && d->Ho == d->Hi && d->Wo == d->Wi;
    const bool half = d->sH == 2 && d->sW == 2 && d->Hi == 2 * d->Ho && d->Wi == 2 * d->Wo;
    if (d->sT != 1 || d->To != d->Ti || !(unit || half)) return w;
    if (d->Ci % 8 || d->Ci > 128 || d->Co % 32 || d->Co > 256) return w;
    if (in_affine || !mask_bits) return w;
    w.cip = d->Ci <= 16 ? 16 : d->Ci <= 32 ? 32 : d->Ci <= 64 ? 64 : 128;
    w.cop = d->Co <= 32 ? 32 : d->Co <= 64 ? 64 : d->Co <= 128 ? 128 : 256;
    int rps;
    const int wgs = cbwd_deal_rows(d, (int64_t)d->N * d->To * d->Ho * d->Wo, &rps);
    if (wgs > SF_CBWD_MAX_WGS) return w;
    w.R = 128;
    w.ws_bytes = (size_t)wgs * w.cop * w.cip * 4;
    w.ok = true;
    return w;
}

extern "C" int sf_conv_proj_bwd_plan(const sf_conv_desc* d, int in_affine, int mask_bits, int64_t* workspace_bytes) {
    if (check_desc(d)) return -1;
    const CbwdPlan w = plan_proj_bwd(d, in_affine != 0, mask_bits != 0);
    if (workspace_bytes) *workspace_bytes = w.ok ? (int64_t)w.ws_bytes : 0;
    return w.ok ? 1 : 0;
}

extern "C" int sf_conv_proj_bwd(const sf_conv_desc* d, const void* dz, int32_t lddz, const void* mask_bits, const void* y1,
                                int32_t ldy1, const float* coef, const void* x, const void* wd, void* d_in, int32_t ld_in,
                                float* dw, float out_scale, int zero_first, void* workspace, int64_t workspace_bytes,
                                sf_stream_t stream) {
    if (check_desc(d)) return -1;
    REQUIRE(dz && mask_bits && y1 && coef && x && wd && d_in && dw && workspace, "sf_conv_proj_bwd: null pointer");
    const CbwdPlan w = plan_proj_bwd(d, false, true);
    REQUIRE(w.ok, "sf_conv_proj_bwd: this geometry keeps sf_bn_bwd_apply + sf_conv_wgrad + sf_conv_dgrad (sf_conv_proj_bwd_plan == 0)");
    REQUIRE(lddz >= d->Co && lddz % 8 == 0 && ldy1 >= d->Co && ldy1 % 8 == 0 && ld_in >= d->Ci && ld_in % 8 == 0 &&
            d->ldx >= d->Ci && d->ldx % 8 == 0, "sf_conv_proj_bwd: bad row pitch");
    REQUIRE((((uintptr_t)dz | (uintptr_t)y1 | (uintptr_t)x | (uintptr_t)wd | (uintptr_t)d_in | (uintptr_t)workspace) & 15) == 0,
            "sf_conv_proj_bwd: operands must be 16-byte aligned");
    REQUIRE(workspace_bytes >= (int64_t)w.ws_bytes, "sf_conv_proj_bwd: workspace too small (%lld < %lld bytes)",
            (long long)workspace_bytes, (long long)w.ws_bytes);
    const int64_t M = (int64_t)d->N * d->To * d->Ho * d->Wo;       // output rows; d_in has d->N * d->Ti * d->Hi * d->Wi
    int32_t ldf, ldd;
    sf_conv_weight_ld(d, &ldf, &ldd);
    CbwdParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.Ci = d->Ci; p.Co = d->Co;
    p.dz = (const f16*)dz; p.lddz = lddz; p.bits = (const uint8_t*)mask_bits; p.yc = (const f16*)y1; p.ldyc = ldy1;
    p.coef = coef; p.act = (const f16*)x; p.ldact = d->ldx; p.wd = (const f16*)wd; p.ldw = ldd;
    p.dx = (f16*)d_in; p.lddx = ld_in; p.ws = (float*)workspace; p.tiles128 = cdiv(M, 128);
    p.str2 = d->sH == 2 ? 1 : 0; p.fdWo = make_fastdiv(d->Wo);
    const int wgs = cbwd_deal_rows(d, M, &p.rps);
    hipStream_t s = (hipStream_t)stream;
    SF_CBWD_FOR_SHAPE(w.cip, w.cop, hipLaunchKernelGGL((sf_cbwd_kernel<CIP_, COP_>), dim3(wgs), dim3(SF_THREADS), 0, s, p));
    if (check_launch("conv_proj_bwd")) return -1;
    launch_wgrad_reduce(d, (const float*)workspace, wgs, w.cop, w.cip, false, dw, out_scale, zero_first, s);
    return check_launch("conv_proj_bwd_reduce");
}

// ------------------------------------------------------------------------------------------------
static RowTile make_rowtile(int64_t M, int C, int max_blocks, dim3& grid) {
    RowTile rt;
    rt.M = (int)M; rt.C = C;
    const int G = C / 8;
    const int TG = G < SF_THREADS ? G : SF_THREADS;
    const int rpi = SF_THREADS / TG;
    int passes = cdiv(M, (int64_t)rpi * max_blocks);
    if (passes < 1) passes = 1;
    rt.rows_per_block = rpi * passes;
    grid = dim3(cdiv(M, rt.rows_per_block), cdiv(G, SF_THREADS));
    return rt;
}
static int check_rows(const char* who, int64_t M, int C) {
    REQUIRE(M > 0 && M < (1ll << 31), "%s: bad row count", who);
    REQUIRE(C > 0 && C % 8 == 0, "%s: C must be a positive multiple of 8 (got %d)", who, C);
    return 0;
}

// Folds a long partial table in place (sf_part_fold_kernel) so that the single-workgroup-per-32-channels
// finalize kernels never walk more than a few hundred rows; returns the row stride of the surviving rows.
// Tables up to kFoldAbove rows are finalized directly by a 1024-thread block per 8 channels (<= 16 rows per thread:
// 7.5 us for the 1024-row tables of the backward pass against 5 + 5 us for fold + finalize); longer tables (the per-tile
// partials of a forward convolution over 800k positions) measured no faster that way and keep the fold stage.
static const int kFoldAbove = tune_knob("SF_FOLD_ABOVE", 2048);
static int fold_partials(float* part, int& nblk, int C, hipStream_t s) {
    if (nblk <= kFoldAbove || nblk <= 256) return 1;
    const int group = nblk <= 2048 ? 16 : nblk <= 8192 ? 32 : 64;
    const int cols = 2 * C;
    dim3 grid(cdiv(cols, SF_THREADS), cdiv(nblk, group));
    hipLaunchKernelGGL(sf_part_fold_kernel, grid, dim3(SF_THREADS), 0, s, part, nblk, cols, group);
    nblk = cdiv(nblk, group);
    return group;
}

extern "C" int sf_bn_finalize(float* part, int32_t nblk, int32_t C, int32_t Creal, float count, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                              float* scale, float* shift, float* save_mean, float* save_rstd, sf_stream_t stream) {
    REQUIRE(gamma && beta && scale && shift, "sf_bn_finalize: null pointer");
    REQUIRE(nblk > 0 ? part != nullptr : (running_mean && running_var), "sf_bn_finalize: missing statistics source");
    REQUIRE(Creal > 0 && Creal <= C, "sf_bn_finalize: Creal must be in (0, C]");
    BnFinalizeParams p;
    p.row_stride = nblk > 0 ? fold_partials(part, nblk, C, (hipStream_t)stream) : 1;
    p.part = part; p.nblk = nblk; p.C = C; p.Creal = Creal; p.count = count; p.gamma = gamma; p.beta = beta;
    p.running_mean = running_mean; p.running_var = running_var; p.momentum = momentum; p.eps = eps;
    p.scale = scale; p.shift = shift; p.save_mean = save_mean; p.save_rstd = save_rstd;
    hipLaunchKernelGGL(sf_bn_finalize_kernel, dim3(cdiv(C, SF_FIN_CH)), dim3(sf_fin_threads(p.nblk)), 0, (hipStream_t)stream, p);
    return check_launch("bn_finalize");
}

extern "C" int sf_bn_act(int64_t M, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                         const void* r, int32_t ldr, const float* rscale, const float* rshift, int relu, void* out,
                         int32_t ldo, void* mask_out, sf_stream_t stream) {
    if (check_rows("sf_bn_act", M, C)) return -1;
    REQUIRE(y && out, "sf_bn_act: null pointer");
    BnActParams p;
    dim3 grid;
    p.rt = make_rowtile(M, C, 8192, grid);
    p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift;
    p.r = (const f16*)r; p.ldr = ldr; p.rscale = rscale; p.rshift = rshift;
    p.relu = relu; p.out = (f16*)out; p.ldo = ldo; p.mask_out = (uint8_t*)mask_out;
    hipLaunchKernelGGL(sf_bn_act_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("bn_act");
}

// row blocks of the BatchNorm-backward reduce (= rows of its partial table); SF_BN_BWD_BLOCKS is an A/B knob
static const int kBwdBlocks = tune_knob("SF_BN_BWD_BLOCKS", 1024);
extern "C" int sf_bn_bwd_blocks(int64_t M, int32_t C) {
    if (check_rows("sf_bn_bwd_blocks", M, C)) return -1;
    dim3 grid;
    make_rowtile(M, C, kBwdBlocks, grid);
    return (int)grid.x;
}

extern "C" int sf_bn_bwd_reduce(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* zmask, int32_t ldm,
                                const void* y, int32_t ldy, const float* scale, const float* shift, int relu_self,
                                float* part, sf_stream_t stream) {
    if (check_rows("sf_bn_bwd_reduce", M, C)) return -1;
    REQUIRE(dz && y && part, "sf_bn_bwd_reduce: null pointer");
    REQUIRE(!relu_self || (scale && shift), "sf_bn_bwd_reduce: relu_self needs scale/shift");
    BnBwdReduceParams p;
    dim3 grid;
    p.rt = make_rowtile(M, C, kBwdBlocks, grid);
    p.dz = (const f16*)dz; p.lddz = lddz; p.zmask = (const f16*)zmask; p.ldm = ldm;
    p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.relu_self = relu_self; p.part = part;
    hipLaunchKernelGGL(sf_bn_bwd_reduce_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("bn_bwd_reduce");
}

extern "C" int sf_bn_bwd_finalize(float* part, int32_t nblk, int32_t C, int32_t Creal, float count, const float* gamma,
                                  const float* mean, const float* rstd, float inv_loss_scale, float* dgamma,
                                  float* dbeta, int accumulate, float* coef, sf_stream_t stream) {
    REQUIRE(part && gamma && mean && rstd && dgamma && dbeta && coef, "sf_bn_bwd_finalize: null pointer");
    BnBwdFinalizeParams p;
    p.row_stride = fold_partials(part, nblk, C, (hipStream_t)stream);
    REQUIRE(Creal > 0 && Creal <= C, "sf_bn_bwd_finalize: Creal must be in (0, C]");
    p.part = part; p.nblk = nblk; p.C = C; p.Creal = Creal; p.count = count; p.gamma = gamma; p.mean = mean; p.rstd = rstd;
    p.inv_loss_scale = inv_loss_scale; p.dgamma = dgamma; p.dbeta = dbeta; p.accumulate = accumulate; p.coef = coef;
    hipLaunchKernelGGL(sf_bn_bwd_finalize_kernel, dim3(cdiv(C, SF_FIN_CH)), dim3(sf_fin_threads(p.nblk)), 0, (hipStream_t)stream, p);
    return check_launch("bn_bwd_finalize");
}

extern "C" int sf_bn_bwd_apply(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* zmask, int32_t ldm,
                               const void* y, int32_t ldy, const float* scale, const float* shift, int relu_self,
                               const float* coef, void* dy, int32_t lddy, void* gout, int32_t ldg,
                               sf_stream_t stream) {
    if (check_rows("sf_bn_bwd_apply", M, C)) return -1;
    REQUIRE(dz && y && coef && dy, "sf_bn_bwd_apply: null pointer");
    REQUIRE(!relu_self || (scale && shift), "sf_bn_bwd_apply: relu_self needs scale/shift");
    BnBwdApplyParams p;
    dim3 grid;
    p.rt = make_rowtile(M, C, 8192, grid);
    p.dz = (const f16*)dz; p.lddz = lddz; p.zmask = (const f16*)zmask; p.ldm = ldm;
    p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.relu_self = relu_self;
    p.coef = coef; p.dy = (f16*)dy; p.lddy = lddy; p.gout = (f16*)gout; p.ldg = ldg;
    p.sample_add = nullptr; p.fdS = make_fastdiv(1);
    hipLaunchKernelGGL(sf_bn_bwd_apply_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("bn_bwd_apply");
}
// ... for a gradient dz that lacks a per-sample constant: dy = k1 * (dz + sample_add[row / S][c]) + k2 + k3 * y (the sums behind
// coef must be those of the COMPLETE gradient).  X3DTransform: the SE squeeze's contribution dmean[n][c] / S (operators.py:38-45)
extern "C" int sf_bn_bwd_apply_sample(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* y, int32_t ldy,
                                      const float* coef, const float* sample_add, int64_t S, void* dy, int32_t lddy,
                                      sf_stream_t stream) {
    if (check_rows("sf_bn_bwd_apply_sample", M, C)) return -1;
    REQUIRE(dz && y && coef && dy && sample_add, "sf_bn_bwd_apply_sample: null pointer");
    REQUIRE(S > 0 && S < (1ll << 31) && M % S == 0, "sf_bn_bwd_apply_sample: rows must be whole samples of S positions");
    BnBwdApplyParams p;
    dim3 grid;
    p.rt = make_rowtile(M, C, 8192, grid);
    p.dz = (const f16*)dz; p.lddz = lddz; p.zmask = nullptr; p.ldm = 0;
    p.y = (const f16*)y; p.ldy = ldy; p.scale = nullptr; p.shift = nullptr; p.relu_self = 0;
    p.coef = coef; p.dy = (f16*)dy; p.lddy = lddy; p.gout = nullptr; p.ldg = 0;
    p.sample_add = sample_add; p.fdS = make_fastdiv((uint32_t)S);
    hipLaunchKernelGGL(sf_bn_bwd_apply_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("bn_bwd_apply_sample");
}

// ------------------------------------------------------------------------------------------------
static int fill_pool(PoolParams& p, int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kH, int32_t kW,
                     int32_t sH, int32_t sW, int32_t pH, int32_t pW, const void* y, int32_t ldy, const float* scale,
                     const float* shift, int relu) {
    REQUIRE(C > 0 && C % 8 == 0, "pool: C must be a multiple of 8");
    REQUIRE((scale == nullptr) == (shift == nullptr), "pool: scale/shift must come together");
    memset(&p, 0, sizeof(p));
    p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.relu = relu;
    p.N = N; p.T = T; p.H = H; p.W = W; p.C = C;
    p.kH = kH; p.kW = kW; p.sH = sH; p.sW = sW; p.pH = pH; p.pW = pW;
    p.Ho = (H + 2 * pH - kH) / sH + 1;
    p.Wo = (W + 2 * pW - kW) / sW + 1;
    p.fdG = make_fastdiv(C / 8);
    return 0;
}
static int pool_grid(int64_t total) {
    int64_t b = (total + SF_THREADS - 1) / SF_THREADS;
    return (int)(b > 65536 ? 65536 : b);
}

extern "C" int sf_pool_fwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kH, int32_t kW, int32_t sH,
                           int32_t sW, int32_t pH, int32_t pW, const void* y, int32_t ldy, const float* scale,
                           const float* shift, int relu, void* out, int32_t ldo, void* argmax, int32_t cls,
                           sf_stream_t stream) {
    PoolParams p;
    if (fill_pool(p, N, T, H, W, C, kH, kW, sH, sW, pH, pW, y, ldy, scale, shift, relu)) return -1;
    REQUIRE(y && out, "sf_pool_fwd: null pointer");
    p.cls = cls ? 1 : 0; p.fdT = make_fastdiv(T);
    REQUIRE(kH * kW <= 255, "sf_pool_fwd: window too large for the byte argmax");
    p.out = (f16*)out; p.ldo = ldo; p.argmax = (uint8_t*)argmax;
    p.fdW = make_fastdiv(p.Wo); p.fdH = make_fastdiv(p.Ho);
    p.total = (int64_t)N * T * p.Ho * p.Wo * (C / 8);
    REQUIRE(p.total < (1ll << 31), "sf_pool_fwd: too many elements");
    hipLaunchKernelGGL(sf_pool_fwd_kernel, dim3(pool_grid(p.total + (int64_t)N * (C / 8))), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("pool_fwd");
}

extern "C" int sf_pool_bwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kH, int32_t kW, int32_t sH,
                           int32_t sW, int32_t pH, int32_t pW, const void* pooled, int32_t ldp, const void* argmax,
                           int relu, const void* dout, int32_t lddo, void* g, int32_t ldg, int32_t cls,
                           sf_stream_t stream) {
    PoolParams p;
    if (fill_pool(p, N, T, H, W, C, kH, kW, sH, sW, pH, pW, nullptr, 0, nullptr, nullptr, relu)) return -1;
    REQUIRE(argmax && dout && g, "sf_pool_bwd: null pointer");           // pooled: not read since round 6 (the ReLU test is in the argmax code)
    (void)pooled; (void)ldp;
    p.cls = cls ? 1 : 0; p.fdT = make_fastdiv(T);
    p.out = (f16*)g; p.ldo = ldg; p.dout = (const f16*)dout; p.lddo = lddo;
    p.pooled = (const f16*)pooled; p.ldp = ldp; p.argmax = (uint8_t*)argmax;
    p.fdW = make_fastdiv(W); p.fdH = make_fastdiv(H);
    p.total = (int64_t)N * T * H * W * (C / 8);
    REQUIRE(p.total < (1ll << 31), "sf_pool_bwd: too many elements");
    p.fdsH = make_fastdiv(sH); p.fdsW = make_fastdiv(sW);
    if (kH <= 2 * sH && kW <= 2 * sW)      // at most 2 x 2 windows cover a position (sf_pool.h)
        hipLaunchKernelGGL(sf_pool_bwd4_kernel, dim3(pool_grid(p.total + (int64_t)N * (C / 8))), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(sf_pool_bwd_kernel, dim3(pool_grid(p.total + (int64_t)N * (C / 8))), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p);
    return check_launch("pool_bwd");
}

// ---- MaxPool3d(kernel = stride, padding 0) of the Nonlocal block (nonlocal_helper.py:96-101)
extern "C" int sf_pool3d_fwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kT, int32_t kH, int32_t kW,
                             const void* x, int32_t ldx, void* out, int32_t ldo, void* argmax, sf_stream_t stream) {
    REQUIRE(x && out && argmax && C > 0 && C % 8 == 0 && kT > 0 && kH > 0 && kW > 0 && kT * kH * kW <= 255,
            "sf_pool3d_fwd: bad arguments");
    Pool3dParams p;
    p.N = N; p.T = T; p.H = H; p.W = W; p.C = C; p.kT = kT; p.kH = kH; p.kW = kW;
    p.To = T / kT; p.Ho = H / kH; p.Wo = W / kW;
    REQUIRE(p.To > 0 && p.Ho > 0 && p.Wo > 0, "sf_pool3d_fwd: window larger than the input");
    p.x = (const f16*)x; p.ldx = ldx; p.out = (f16*)out; p.ldo = ldo; p.argmax = (uint8_t*)argmax;
    p.dout = nullptr; p.lddo = 0;
    p.fdG = make_fastdiv(C / 8); p.fdW = make_fastdiv(p.Wo); p.fdH = make_fastdiv(p.Ho); p.fdT = make_fastdiv(p.To);
    p.total = (int64_t)N * p.To * p.Ho * p.Wo * (C / 8);
    REQUIRE(p.total < (1ll << 31), "sf_pool3d_fwd: too many elements");
    hipLaunchKernelGGL(sf_pool3d_fwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("pool3d_fwd");
}
extern "C" int sf_pool3d_bwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kT, int32_t kH, int32_t kW,
                             const void* argmax, const void* dout, int32_t lddo, void* dx, int32_t lddx, sf_stream_t stream) {
    REQUIRE(argmax && dout && dx && C > 0 && C % 8 == 0 && kT > 0 && kH > 0 && kW > 0, "sf_pool3d_bwd: bad arguments");
    Pool3dParams p;
    p.N = N; p.T = T; p.H = H; p.W = W; p.C = C; p.kT = kT; p.kH = kH; p.kW = kW;
    p.To = T / kT; p.Ho = H / kH; p.Wo = W / kW;
    p.x = nullptr; p.ldx = 0; p.out = (f16*)dx; p.ldo = lddx; p.argmax = (uint8_t*)argmax;
    p.dout = (const f16*)dout; p.lddo = lddo;
    p.fdG = make_fastdiv(C / 8); p.fdW = make_fastdiv(W); p.fdH = make_fastdiv(H); p.fdT = make_fastdiv(T);
    p.total = (int64_t)N * T * H * W * (C / 8);
    REQUIRE(p.total < (1ll << 31), "sf_pool3d_bwd: too many elements");
    hipLaunchKernelGGL(sf_pool3d_bwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("pool3d_bwd");
}

extern "C" int sf_ncthw_to_cl(const float* x, int32_t N, int32_t C, int64_t S, int32_t Cp, void* out,
                              sf_stream_t stream) {
    REQUIRE(x && out && (Cp % 8 == 0 || Cp == 4) && Cp >= C, "sf_ncthw_to_cl: bad arguments");
    static const bool quad = test_hook("SF_LAYOUT_QUAD", 1) != 0;
    if (quad && C <= 4 && Cp <= 8 && S % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {   // RGB clips: four positions per lane
        const int grid = pool_grid((int64_t)N * (S / 4));
        if (Cp == 4) hipLaunchKernelGGL(sf_ncthw_to_cl_quad_kernel<4>, dim3(grid), dim3(SF_THREADS), 0, (hipStream_t)stream, x, (f16*)out, N, C, S / 4);
        else hipLaunchKernelGGL(sf_ncthw_to_cl_quad_kernel<8>, dim3(grid), dim3(SF_THREADS), 0, (hipStream_t)stream, x, (f16*)out, N, C, S / 4);
        return check_launch("ncthw_to_cl");
    }
    hipLaunchKernelGGL(sf_ncthw_to_cl_kernel, dim3(pool_grid((int64_t)N * S)), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, x, (f16*)out, N, C, S, Cp);
    return check_launch("ncthw_to_cl");
}

extern "C" int sf_cl_to_ncthw(const void* x, int32_t ld, int32_t N, int32_t C, int64_t S, float* out,
                              sf_stream_t stream) {
    REQUIRE(x && out && ld >= C, "sf_cl_to_ncthw: bad arguments");
    hipLaunchKernelGGL(sf_cl_to_ncthw_kernel, dim3(pool_grid((int64_t)N * C * S)), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, (const f16*)x, ld, out, N, C, S);
    return check_launch("cl_to_ncthw");
}

// ================================================================================================
// Token-space entry points (MViT / Nonlocal / X3D): batched GEMMs, LayerNorm, GELU, column sums, depthwise
// convolution, pooled-attention softmax with relative-position bias.
static GatherSide gather_matrix(const void* a, int64_t M, int32_t K, int32_t lda) {
    // a plain [M][K] matrix as the pointwise gather of a 1x1x1 convolution over N=1, T=1, H=1, W=M
    GatherSide g;
    memset(&g, 0, sizeof(g));
    g.src = (const f16*)a; g.ld = lda; g.C = K;
    g.sT = 1; g.sH = 1; g.sW = (int)M;
    g.kT = g.kH = g.kW = 1; g.strT = g.strH = g.strW = 1; g.dilT = g.dilH = g.dilW = 1;
    g.mode = 0; g.Ktot = K;
    g.fdC = make_fastdiv(K); g.fdkW = make_fastdiv(1); g.fdkH = make_fastdiv(1);
    g.fdrW = make_fastdiv((uint32_t)M); g.fdrH = make_fastdiv(1); g.fdrT = make_fastdiv(1);
    g.fdsT = g.fdsH = g.fdsW = make_fastdiv(1);
    g.fdHW = make_fastdiv((uint32_t)M); g.rowT = 1;
    return g;
}

// sf_rows32 -> the kernels' F32Rows (need_out: the entry point writes side rows; otherwise it only reads them)
static int rows32_arg(const char* who, const sf_rows32* side, int64_t M, int32_t C, bool need_out, F32Rows& f) {
    memset(&f, 0, sizeof(f));
    if (!side) return 0;
    REQUIRE(side->period >= 1 && side->ld >= C && side->ld % 4 == 0, "%s: bad side rows (period %d, ld %d, C %d)", who,
            side->period, side->ld, C);
    REQUIRE(need_out ? side->out != nullptr : side->in != nullptr, "%s: side rows without a buffer", who);
    REQUIRE(((uintptr_t)side->in | (uintptr_t)side->out) % 16 == 0, "%s: side rows need 16-byte bases", who);
    f.in = side->in; f.out = side->out; f.ld = side->ld; f.fd = make_fastdiv((uint32_t)side->period);
    (void)M;
    return 0;
}

static int bgemm_impl(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                      const float* bias, const void* resid, int32_t ldr, void* Y, int32_t ldy, int32_t nbatch,
                      int32_t bh, int64_t sa_b, int64_t sa_h, int64_t sw_b, int64_t sw_h, int64_t sy_b, int64_t sy_h,
                      int64_t sr_b, int64_t sr_h, int32_t resid_row0, float alpha, const sf_rows32* side, sf_stream_t stream) {
    REQUIRE(A && W && Y, "sf_bgemm: null pointer");
    REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "sf_bgemm: bad shape");
    // rows of Y are written in 16-byte groups: the pitch must cover N rounded up to 8 (the pad columns get zeros)
    REQUIRE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 && lda >= K && ldw >= K && ldy >= roundup(N, 8),
            "sf_bgemm: K and the pitches must be multiples of 8 (N=%d K=%d lda=%d ldw=%d ldy=%d)", N, K, lda, ldw, ldy);
    REQUIRE(!(bias || resid) || N % 8 == 0, "sf_bgemm: bias / residual need N %% 8 == 0");
    REQUIRE(nbatch >= 1 && bh >= 1 && nbatch % bh == 0 && nbatch <= 65535, "sf_bgemm: bad batch (%d, %d)", nbatch, bh);
    REQUIRE(!resid || (ldr % 8 == 0 && ldr >= N), "sf_bgemm: bad residual pitch");
    IgemmParams p = gemm_params(gather_matrix(A, M, K, lda), (int)M, W, ldw, N, Y, ldy, bias, resid, ldr);
    p.bh = bh; p.sa_b = sa_b; p.sa_h = sa_h; p.sw_b = sw_b; p.sw_h = sw_h; p.sy_b = sy_b; p.sy_h = sy_h;
    p.linear = 1;
    p.sr_b = sr_b; p.sr_h = sr_h; p.resid_row0 = resid_row0; p.alpha = alpha;
    if (side) {
        REQUIRE(nbatch == 1 && N % 8 == 0, "sf_gemm_rows32: one GEMM, N %% 8 == 0 (N=%d)", N);
        if (rows32_arg("sf_gemm_rows32", side, M, N, true, p.f32)) return -1;
    }
    const GemmPlan g = plan_gemm(p, true, nbatch);
    launch_gemm(g, p, (hipStream_t)stream);
    return check_launch(g.kind == GEMM_GEN2 ? "bgemm2" : "bgemm");
}

extern "C" int sf_bgemm(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                        const float* bias, const void* resid, int32_t ldr, void* Y, int32_t ldy, int32_t nbatch,
                        int32_t bh, int64_t sa_b, int64_t sa_h, int64_t sw_b, int64_t sw_h, int64_t sy_b, int64_t sy_h,
                        int64_t sr_b, int64_t sr_h, int32_t resid_row0, float alpha, sf_stream_t stream) {
    return bgemm_impl(M, N, K, A, lda, W, ldw, bias, resid, ldr, Y, ldy, nbatch, bh, sa_b, sa_h, sw_b, sw_h, sy_b, sy_h, sr_b,
                      sr_h, resid_row0, alpha, nullptr, stream);
}

extern "C" int sf_gemm_rows32(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                              const float* bias, const void* resid, int32_t ldr, void* Y, int32_t ldy,
                              const sf_rows32* side, sf_stream_t stream) {
    REQUIRE(side, "sf_gemm_rows32: null side rows");
    return bgemm_impl(M, N, K, A, lda, W, ldw, bias, resid, ldr, Y, ldy, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.f, side, stream);
}

static int gemm_act_impl(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                         const float* bias, void* Y, int32_t ldy, int32_t mode, void* aux, int32_t ldaux,
                         float* colsum_part, int32_t* colsum_rows, sf_stream_t stream) {
    REQUIRE(A && W && Y && aux, "sf_gemm_act: null pointer");
    REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "sf_gemm_act: bad shape");
    REQUIRE(N % 8 == 0 && K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 && ldaux % 8 == 0 && ldaux >= N,
            "sf_gemm_act: N, K and the pitches must be multiples of 8");
    REQUIRE(mode == 1 || mode == 2, "sf_gemm_act: mode must be 1 (write gelu(y)) or 2 (multiply by gelu'(aux))");
    IgemmParams p = gemm_params(gather_matrix(A, M, K, lda), (int)M, W, ldw, N, Y, ldy, bias, nullptr, 0);
    p.bh = 1;
    p.act_mode = mode; p.act_aux = (f16*)aux; p.ld_aux = ldaux;
    p.linear = 1;
    p.bnb_part = colsum_part;          // bnb_y == nullptr: plain column sums of the stored tile, one row per M tile
    const GemmPlan g = plan_gemm(p, true, 1);
    if (colsum_rows) *colsum_rows = colsum_part ? cdiv(p.M, g.bm) : 0;
    launch_gemm(g, p, (hipStream_t)stream);
    return check_launch(g.kind == GEMM_GEN2 ? "gemm_act2" : "gemm_act");
}

extern "C" int sf_gemm_act(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                           const float* bias, void* Y, int32_t ldy, int32_t mode, void* aux, int32_t ldaux,
                           sf_stream_t stream) {
    return gemm_act_impl(M, N, K, A, lda, W, ldw, bias, Y, ldy, mode, aux, ldaux, nullptr, nullptr, stream);
}

extern "C" int sf_gemm_act_colsum(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                                  const float* bias, void* Y, int32_t ldy, int32_t mode, void* aux, int32_t ldaux,
                                  float* colsum_part, int32_t colsum_part_rows, int32_t* colsum_rows, sf_stream_t stream) {
    REQUIRE(colsum_part && colsum_rows, "sf_gemm_act_colsum: null pointer");
    REQUIRE((int64_t)colsum_part_rows * 128 >= M, "sf_gemm_act_colsum: colsum_part needs ceil(M / 128) rows of [2][N] floats");
    return gemm_act_impl(M, N, K, A, lda, W, ldw, bias, Y, ldy, mode, aux, ldaux, colsum_part, colsum_rows, stream);
}

extern "C" int sf_bgemm_tn(int64_t M, int32_t R, int32_t Kc, const void* P, int32_t ldp, const void* X, int32_t ldx,
                           void* Out, int32_t ldo, float scale, int32_t nbatch, int32_t bh, int64_t sp_b, int64_t sp_h,
                           int64_t sx_b, int64_t sx_h, int64_t so_b, int64_t so_h, sf_stream_t stream) {
    REQUIRE(P && X && Out, "sf_bgemm_tn: null pointer");
    REQUIRE(M > 0 && M < (1ll << 31) && R > 0 && Kc > 0, "sf_bgemm_tn: bad shape");
    REQUIRE(Kc % 8 == 0 && ldp % 8 == 0 && ldx % 8 == 0 && ldp >= R && ldx >= Kc && ldo >= Kc,
            "sf_bgemm_tn: Kc and the pitches must be multiples of 8");
    REQUIRE(nbatch >= 1 && bh >= 1 && nbatch % bh == 0 && nbatch <= 65535, "sf_bgemm_tn: bad batch");
    WgradParams p;
    memset(&p, 0, sizeof(p));
    p.g = gather_matrix(X, M, Kc, ldx);
    p.dy = (const f16*)P; p.ldy = ldp; p.Co = R; p.M = (int)M;
    p.nchunks = cdiv(M, 32);
    p.bh = bh; p.sp_b = sp_b; p.sp_h = sp_h; p.sx_b = sx_b; p.sx_h = sx_h; p.so_b = so_b; p.so_h = so_h;
    p.out16 = (f16*)Out; p.ldo = ldo; p.out_scale = scale;
    const int bmw = wgrad1_bmw(R);
    p.chunks_per_split = roundup(p.nchunks, wgrad1_ks(bmw));        // one split of whole stages
    launch_wgrad1(bmw, p, dim3(cdiv(Kc, 128), cdiv(R, bmw), nbatch), (hipStream_t)stream);
    return check_launch("bgemm_tn");
}

// ---- LayerNorm
template <int L, int NS>
static void launch_ln_fwd(const LnParams& p, hipStream_t s) {
    // rows in flight per thread: 2 for the one- and three-slot rows (SF_LN_RU=1 keeps one, A/B runs)
    static const int ru_env = tune_knob("SF_LN_RU", 2);
    constexpr int RU2 = NS != 2 ? 2 : 1;
    const int ru = ru_env != 1 ? RU2 : 1;
    // 2048 workgroups (= the chip's 8 waves per SIMD once over) walking the rows: 68 / 39 / 27.5 us at the MViTv2-S block-0 /
    // stage-2 / stage-3 shapes against 73 / 44 / 36 us with 4096 and 81 / 58 / 45 us with 8192 (profiles/r4/r4_v17_ln_fwd_blocks.txt)
    static const int max_blocks = tune_knob("SF_LN_FWD_BLOCKS", 2048);
    const int rpb = SF_THREADS / L * ru;
    int blocks = cdiv(p.M, rpb);
    if (blocks > max_blocks) blocks = max_blocks;
    if (ru == 2) hipLaunchKernelGGL((sf_layernorm_fwd_kernel<L, NS, RU2>), dim3(blocks), dim3(SF_THREADS), 0, s, p);
    else hipLaunchKernelGGL((sf_layernorm_fwd_kernel<L, NS, 1>), dim3(blocks), dim3(SF_THREADS), 0, s, p);
}
static int ln_bwd_ru() {
    static const int ru = tune_knob("SF_LN_BWD_RU", 2);
    return ru;
}
template <int L, int NS>
static void launch_ln_bwd(const LnParams& p, int blocks, hipStream_t s) {
    // rows in flight per thread: 2 for the one-slot rows (SF_LN_BWD_RU=1 keeps one, A/B runs)
    if (NS == 1 && ln_bwd_ru() != 1) hipLaunchKernelGGL((sf_layernorm_bwd_kernel<L, NS, NS == 1 ? 2 : 1>), dim3(blocks), dim3(SF_THREADS), 0, s, p);
    else hipLaunchKernelGGL((sf_layernorm_bwd_kernel<L, NS, 1>), dim3(blocks), dim3(SF_THREADS), 0, s, p);
}
static int ln_lanes(int C) { return C <= 128 ? 16 : C <= 256 ? 32 : 64; }
static int check_ln(const char* who, int64_t M, int C) {
    REQUIRE(M > 0 && M < (1ll << 31), "%s: bad row count", who);
    REQUIRE(C > 0 && C % 8 == 0 && C <= 1024, "%s: C must be a multiple of 8, <= 1024 (got %d)", who, C);
    return 0;
}
static int layernorm_fwd_impl(int64_t M, int32_t C, const void* x, int32_t ldx, const float* gamma, const float* beta,
                              float eps, void* y, int32_t ldy, float* mean, float* rstd, const sf_rows32* side,
                              sf_stream_t stream) {
    if (check_ln("sf_layernorm_fwd", M, C)) return -1;
    REQUIRE(x && gamma && beta && y, "sf_layernorm_fwd: null pointer");
    LnParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.C = C; p.x = (const f16*)x; p.ldx = ldx; p.gamma = gamma; p.beta = beta; p.eps = eps;
    p.y = (f16*)y; p.ldy = ldy; p.mean = mean; p.rstd = rstd;
    if (rows32_arg("sf_layernorm_fwd_rows32", side, M, C, false, p.f32)) return -1;
    hipStream_t s = (hipStream_t)stream;
    // C = 768: three 8-channel slots on 32 lanes (no idle lanes, 8 rows per workgroup pass) instead of two slots on 64 lanes
    // with a quarter of them idle: 41.6 -> 30.8 us at M = 12576.  The same idea at C = 96 / 192 / 384 (4 / 8 / 16 lanes x three
    // slots) is SLOWER than the power-of-two lane counts with idle lanes (72 -> 81, 44 -> 52, 34 -> 49 us): a wave's 16-byte
    // loads then cover 64 / 128 / 256-byte pieces at the row pitch instead of whole rows (profiles/r4/r4_v16_ln_bench.txt).
    if (C == 768) launch_ln_fwd<32, 3>(p, s);
    else if (C <= 128) launch_ln_fwd<16, 1>(p, s);
    else if (C <= 256) launch_ln_fwd<32, 1>(p, s);
    else if (C <= 512) launch_ln_fwd<64, 1>(p, s);
    else launch_ln_fwd<64, 2>(p, s);
    return check_launch("layernorm_fwd");
}
extern "C" int sf_layernorm_fwd(int64_t M, int32_t C, const void* x, int32_t ldx, const float* gamma, const float* beta,
                                float eps, void* y, int32_t ldy, float* mean, float* rstd, sf_stream_t stream) {
    return layernorm_fwd_impl(M, C, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, nullptr, stream);
}
extern "C" int sf_layernorm_fwd_rows32(int64_t M, int32_t C, const void* x, int32_t ldx, const float* gamma,
                                       const float* beta, float eps, void* y, int32_t ldy, float* mean, float* rstd,
                                       const sf_rows32* side, sf_stream_t stream) {
    REQUIRE(side, "sf_layernorm_fwd_rows32: null side rows");
    return layernorm_fwd_impl(M, C, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, side, stream);
}
static int ln_bwd_plan(int64_t M, int C, int& rows_per_block) {
    const int rpb = SF_THREADS / ln_lanes(C);
    // every workgroup resident at once: 256 CUs x 4 (one row in flight, 4 waves per SIMD) or x 3 (two rows, 154 VGPRs)
    static const int env_blocks = tune_knob("SF_LN_BWD_BLOCKS", 0);
    const int max_blocks = env_blocks > 0 ? env_blocks : (C <= 512 && ln_bwd_ru() != 1) ? 768 : 1024;
    int blocks = cdiv(M, rpb);
    if (blocks > max_blocks) blocks = max_blocks;
    rows_per_block = roundup(cdiv(M, blocks), rpb);
    return cdiv(M, rows_per_block);
}
extern "C" int sf_layernorm_bwd_blocks(int64_t M, int32_t C) {
    if (check_ln("sf_layernorm_bwd_blocks", M, C)) return -1;
    int rpb;
    return ln_bwd_plan(M, C, rpb);
}
static int layernorm_bwd_impl(int64_t M, int32_t C, const void* dy, int32_t lddy, const void* x, int32_t ldx,
                              const float* gamma, const float* mean, const float* rstd, const void* resid, int32_t ldr,
                              void* dx, int32_t lddx, float* part, int part_rows, sf_stream_t stream) {
    if (check_ln("sf_layernorm_bwd", M, C)) return -1;
    REQUIRE(dy && x && gamma && mean && rstd && dx && part, "sf_layernorm_bwd: null pointer");
    LnParams p;
    memset(&p, 0, sizeof(p));
    p.part_rows = part_rows;
    p.M = (int)M; p.C = C; p.x = (const f16*)x; p.ldx = ldx; p.gamma = gamma; p.mean = (float*)mean; p.rstd = (float*)rstd;
    p.dy = (const f16*)dy; p.lddy = lddy; p.resid = (const f16*)resid; p.ldr = ldr; p.dx = (f16*)dx; p.lddx = lddx;
    p.part = part;
    const int blocks = ln_bwd_plan(M, C, p.rows_per_block);
    hipStream_t s = (hipStream_t)stream;
    if (C <= 128) launch_ln_bwd<16, 1>(p, blocks, s);
    else if (C <= 256) launch_ln_bwd<32, 1>(p, blocks, s);
    else if (C <= 512) launch_ln_bwd<64, 1>(p, blocks, s);
    else launch_ln_bwd<64, 2>(p, blocks, s);
    return check_launch("layernorm_bwd");
}
extern "C" int sf_layernorm_bwd(int64_t M, int32_t C, const void* dy, int32_t lddy, const void* x, int32_t ldx,
                                const float* gamma, const float* mean, const float* rstd, const void* resid, int32_t ldr,
                                void* dx, int32_t lddx, float* part, sf_stream_t stream) {
    return layernorm_bwd_impl(M, C, dy, lddy, x, ldx, gamma, mean, rstd, resid, ldr, dx, lddx, part, 2, stream);
}
extern "C" int sf_layernorm_bwd_sums(int64_t M, int32_t C, const void* dy, int32_t lddy, const void* x, int32_t ldx,
                                     const float* gamma, const float* mean, const float* rstd, const void* resid, int32_t ldr,
                                     void* dx, int32_t lddx, float* part, sf_stream_t stream) {
    return layernorm_bwd_impl(M, C, dy, lddy, x, ldx, gamma, mean, rstd, resid, ldr, dx, lddx, part, 4, stream);
}

// ---- column sums
static const int kColBlocks = 1024;
extern "C" int sf_colsum_blocks(int64_t M, int32_t C) {
    if (check_rows("sf_colsum_blocks", M, C)) return -1;
    dim3 grid;
    make_rowtile(M, C, kColBlocks, grid);
    return (int)grid.x;
}
extern "C" int sf_colsum(int64_t M, int32_t C, const void* x, int32_t ldx, float* part, sf_stream_t stream) {
    if (check_rows("sf_colsum", M, C)) return -1;
    REQUIRE(x && part, "sf_colsum: null pointer");
    ColSumParams p;
    dim3 grid;
    p.rt = make_rowtile(M, C, kColBlocks, grid);
    p.x = (const f16*)x; p.ldx = ldx; p.part = part;
    hipLaunchKernelGGL(sf_colsum_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("colsum");
}
extern "C" int sf_colsum_finalize(float* part, int32_t nblk, int32_t C, int32_t fold, float* out0, float* out1,
                                  float scale, int accumulate, sf_stream_t stream) {
    REQUIRE(part && nblk > 0 && C > 0 && fold > 0 && C % fold == 0, "sf_colsum_finalize: bad arguments");
    ColFinalizeParams p;
    p.row_stride = fold_partials(part, nblk, C, (hipStream_t)stream);
    p.part = part; p.nblk = nblk; p.C = C; p.fold = fold; p.out0 = out0; p.out1 = out1; p.scale = scale;
    p.accumulate = accumulate;
    hipLaunchKernelGGL(sf_colsum_finalize_kernel, dim3(cdiv(fold, SF_FIN_CH)), dim3(sf_fin_threads(p.nblk)), 0, (hipStream_t)stream, p);
    return check_launch("colsum_finalize");
}

// ---- GELU
extern "C" int sf_colsum_finalize_batch(const sf_colfin_item* items, int32_t n, sf_stream_t stream) {
    REQUIRE(items && n > 0, "sf_colsum_finalize_batch: no items");
    for (int i0 = 0; i0 < n; i0 += SF_COLFIN_BATCH) {
        ColFinalizeBatch b;
        memset(&b, 0, sizeof(b));
        b.n = n - i0 < SF_COLFIN_BATCH ? n - i0 : SF_COLFIN_BATCH;
        int threads = SF_FIN_SEG * SF_FIN_CH;
        for (int i = 0; i < b.n; ++i) {
            const sf_colfin_item& it = items[i0 + i];
            REQUIRE(it.part && it.nblk > 0 && it.C > 0 && it.fold > 0 && it.C % it.fold == 0 && (it.out0 || it.out1),
                    "sf_colsum_finalize_batch: bad item %d", i0 + i);
            REQUIRE(it.nblk <= kFoldAbove || it.nblk <= 256, "sf_colsum_finalize_batch: item %d has %d partial rows (use sf_colsum_finalize)",
                    i0 + i, it.nblk);
            ColFinalizeParams& p = b.item[i];
            REQUIRE(it.row_stride >= 0 && it.row_stride <= 64, "sf_colsum_finalize_batch: bad row stride in item %d", i0 + i);
            p.part = it.part; p.nblk = it.nblk; p.row_stride = it.row_stride > 0 ? it.row_stride : 1; p.C = it.C; p.fold = it.fold;
            p.out0 = it.out0; p.out1 = it.out1;
            p.scale = it.scale; p.accumulate = it.accumulate;
            b.first[i + 1] = b.first[i] + cdiv(it.fold, SF_FIN_CH);
            if (sf_fin_threads(it.nblk) > threads) threads = sf_fin_threads(it.nblk);
        }
        hipLaunchKernelGGL(sf_colsum_finalize_batch_kernel, dim3(b.first[b.n]), dim3(threads), 0, (hipStream_t)stream, b);
    }
    return check_launch("colsum_finalize_batch");
}

extern "C" int sf_gelu_fwd(int64_t n, const void* h, void* a, sf_stream_t stream) {
    REQUIRE(h && a && n > 0 && n % 8 == 0, "sf_gelu_fwd: bad arguments");
    hipLaunchKernelGGL(sf_gelu_fwd_kernel, dim3(pool_grid(n / 8)), dim3(SF_THREADS), 0, (hipStream_t)stream,
                       (const f16*)h, (f16*)a, n / 8);
    return check_launch("gelu_fwd");
}
extern "C" int sf_gelu_bwd(int64_t n, const void* h, const void* da, void* dh, sf_stream_t stream) {
    REQUIRE(h && da && dh && n > 0 && n % 8 == 0, "sf_gelu_bwd: bad arguments");
    hipLaunchKernelGGL(sf_gelu_bwd_kernel, dim3(pool_grid(n / 8)), dim3(SF_THREADS), 0, (hipStream_t)stream,
                       (const f16*)h, (const f16*)da, (f16*)dh, n / 8);
    return check_launch("gelu_bwd");
}

// ---- depthwise convolution
static int fill_dw(DwParams& p, const sf_dw_desc* d, bool rows_are_outputs, int max_blocks, dim3& grid) {
    REQUIRE(d != nullptr, "dwconv: null descriptor");
    REQUIRE(d->N > 0 && d->C > 0 && d->C % 8 == 0 && d->Cw > 0 && d->Cw % 8 == 0 && d->C % d->Cw == 0,
            "dwconv: C and Cw must be multiples of 8 with C %% Cw == 0 (C=%d Cw=%d)", d->C, d->Cw);
    const int taps = d->kT * d->kH * d->kW;
    REQUIRE(taps * d->Cw <= SF_DW_MAX_W, "dwconv: taps*Cw = %d exceeds the LDS weight stage (%d)", taps * d->Cw, SF_DW_MAX_W);
    const int To = (d->Ti + 2 * d->pT - d->kT) / d->sT + 1, Ho = (d->Hi + 2 * d->pH - d->kH) / d->sH + 1,
              Wo = (d->Wi + 2 * d->pW - d->kW) / d->sW + 1;
    REQUIRE(To == d->To && Ho == d->Ho && Wo == d->Wo, "dwconv: output dims do not match the geometry");
    memset(&p, 0, sizeof(p));
    REQUIRE(d->Cwreal >= 0 && d->Cwreal <= d->Cw, "dwconv: Cwreal must be in [0, Cw]");
    p.N = d->N; p.C = d->C; p.Cw = d->Cw; p.Cwreal = d->Cwreal ? d->Cwreal : d->Cw; p.cls = d->cls ? 1 : 0;
    p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi; p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo;
    p.kT = d->kT; p.kH = d->kH; p.kW = d->kW; p.sT = d->sT; p.sH = d->sH; p.sW = d->sW;
    p.pT = d->pT; p.pH = d->pH; p.pW = d->pW;
    const int64_t S = rows_are_outputs ? (int64_t)d->To * d->Ho * d->Wo : (int64_t)d->Ti * d->Hi * d->Wi;
    const int64_t M = (int64_t)d->N * (S + p.cls);
    REQUIRE(M < (1ll << 31), "dwconv: too many rows");
    p.rt = make_rowtile(M, d->C, max_blocks, grid);
    p.fdRow = make_fastdiv((uint32_t)(S + p.cls));
    p.fdW = make_fastdiv(rows_are_outputs ? d->Wo : d->Wi);
    p.fdH = make_fastdiv(rows_are_outputs ? d->Ho : d->Hi);
    p.fdsT = make_fastdiv(d->sT); p.fdsH = make_fastdiv(d->sH); p.fdsW = make_fastdiv(d->sW);
    // row blocks handed out XCD-contiguously (sf_dwconv.h: dw_block_id); SF_DW_XCD=0 keeps the plain order (A/B runs)
    static const bool xcd = tune_knob("SF_DW_XCD", 1) != 0;
    p.xcd_order = xcd ? 1 : 0;
    return 0;
}
static const int kDwFwdBlocks = 2048, kDwWgradBlocks = 256;

// W-blocked kernels: (kW, sW) in {(3,1), (3,2), (1,1)} with pW = kW/2; returns 0 when the geometry is not covered
static int dw_blocked_kind(const sf_dw_desc* d) {
    if (tune_knob("SF_DW_GENERIC", 0) != 0) return 0;
    if (d->pW != d->kW / 2 || d->kH * d->kW > 9) return 0;      // the blocked weight gradient keeps <= 9 taps per plane
    if (d->kW == 3 && d->sW == 1) return 1;
    if (d->kW == 3 && d->sW == 2) return 2;
    if (d->kW == 1 && d->sW == 1 && d->kT * d->kH * d->Cw <= 3072) return 3;
    return 0;
}
// re-plan the RowTile over line groups (4 columns each) of the iterated space + the cls items
static void dw_block_plan(DwParams& p, DwBlockIdx& bi, const sf_dw_desc* d, bool rows_are_outputs, int max_blocks, dim3& grid) {
    const int T = rows_are_outputs ? d->To : d->Ti, H = rows_are_outputs ? d->Ho : d->Hi, W = rows_are_outputs ? d->Wo : d->Wi;
    bi.WG = cdiv(W, SF_DW_WB);
    bi.fdWG = make_fastdiv(bi.WG); bi.fdH = make_fastdiv(H); bi.fdT = make_fastdiv(T);
    bi.groups = (int64_t)d->N * T * H * bi.WG;
    const int64_t items = bi.groups + (p.cls ? d->N : 0);
    p.rt = make_rowtile(items, d->C, max_blocks, grid);
}
#define SF_DW_SMALL_W 3072
// (A one-plane software prefetch in these stencils cost ~90 VGPRs -- 2 instead of 3 waves per SIMD -- and measured slower:
// X3D-M 1092 vs 1137 clips/s, profiles/r1/r1_visit22_ab.txt; removed with the first-version stencils in round 3.)
// forward / data-gradient stencils: fp32 LDS weights for the narrow layers, fp16 for the wide ones
#define SF_DW_DISPATCH_WT(kind, KERNEL, grid, s, p, bi)                                                                 \
    do {                                                                                                                  \
        const bool small_w = (p).kT * (p).kH * (p).kW * (p).Cw <= SF_DW_SMALL_W;                                        \
        if ((kind) == 1 && small_w) hipLaunchKernelGGL((KERNEL<3, 1, SF_DW_SMALL_W, float>), grid, dim3(SF_THREADS), 0, s, p, bi); \
        else if ((kind) == 1) hipLaunchKernelGGL((KERNEL<3, 1, SF_DW_MAX_W, f16>), grid, dim3(SF_THREADS), 0, s, p, bi); \
        else if ((kind) == 2 && small_w) hipLaunchKernelGGL((KERNEL<3, 2, SF_DW_SMALL_W, float>), grid, dim3(SF_THREADS), 0, s, p, bi); \
        else if ((kind) == 2) hipLaunchKernelGGL((KERNEL<3, 2, SF_DW_MAX_W, f16>), grid, dim3(SF_THREADS), 0, s, p, bi); \
        else hipLaunchKernelGGL((KERNEL<1, 1, SF_DW_SMALL_W, float>), grid, dim3(SF_THREADS), 0, s, p, bi);             \
    } while (0)
// ------------------------------------------------------------------------------------------------
// Plane sweeps (sf_dwsweep.h, round 6) of the 3x3x3 / padding 1 / stride (1, s, s) depthwise convolutions (MViT pooling, X3D
// channelwise).  SF_DW_SWEEP=0 keeps the stencils (tests, read per call).
static bool dwsweep_shape_ok(const sf_dw_desc* d) {
    if (d->kT != 3 || d->kH != 3 || d->kW != 3 || d->pT != 1 || d->pH != 1 || d->pW != 1) return false;
    if (d->sT != 1 || d->sH != d->sW || (d->sH != 1 && d->sH != 2) || d->To != d->Ti) return false;
    return d->C % 8 == 0 && d->Cw % 8 == 0;
}
static int64_t dwsweep_max_rows(const sf_dw_desc* d) { return (int64_t)d->N * d->Ho * 4; }
// Stride-2 data gradient on sf_dwsweep_kernel<1, 2, .>: the iterated space is dy (a lane writes the 2 x 2 block of dx above each
// position), the staged tile is dy with a one-row / one-column halo.  SF_DWS_TH / SF_DWS_TW / SF_DWS_NSEG force a tiling (tests).
static bool dwsweep_plan(const sf_dw_desc* d, DwSweepParams& p) {
    if (test_hook("SF_DW_SWEEP", 1) == 0) return false;
    if (!dwsweep_shape_ok(d) || d->sH != 2) return false;
    memset(&p, 0, sizeof(p));
    p.N = d->N; p.C = d->C; p.Cw = d->Cw; p.Cwreal = d->Cwreal ? d->Cwreal : d->Cw; p.cls = d->cls ? 1 : 0; p.T = d->Ti;
    p.nchunks = cdiv(d->C, 32);
    p.Ha = d->Ho; p.Wa = d->Wo; p.Hd = d->Hi; p.Wd = d->Wi; p.Hit = d->Ho; p.Wit = d->Wo;
    const int f_th = test_hook("SF_DWS_TH", 0), f_tw = test_hook("SF_DWS_TW", 0), f_seg = test_hook("SF_DWS_NSEG", 0);
    double best = 0.0;
    for (int kw = 1; kw <= 16; ++kw) {
        const int tw = cdiv(p.Wit, kw);
        if (kw > 1 && tw == cdiv(p.Wit, kw - 1)) continue;
        if (f_tw > 0 && tw != (f_tw < p.Wit ? f_tw : p.Wit)) continue;
        const int ca = tw + 1;
        int rp = ca * 64;
        if (rp % 128 == 0) rp += 64;
        for (int th = p.Hit < 32 ? p.Hit : 32; th >= 1; --th) {
            if (f_th > 0 && th != (f_th < p.Hit ? f_th : p.Hit)) continue;
            const int ra = th + 1;
            const int slotb = roundup(ra * rp, 1024);
            if (slotb > SF_DWS_MAXVPT * 4096 || SF_DWS_NR * slotb > SF_DWS_LDS) continue;
            const int tiles_h = cdiv(p.Hit, th), tiles_w = cdiv(p.Wit, tw);
            if ((int64_t)p.N * tiles_h * tiles_w > dwsweep_max_rows(d)) continue;
            const int ngrp = cdiv(th, 8);
            for (int nseg = 1; nseg <= 8 && nseg <= tw; ++nseg) {
                if (f_seg > 0 && nseg != (f_seg < tw ? f_seg : tw)) continue;
                const int sl = cdiv(tw, nseg);
                if (cdiv(tw, sl) != nseg) continue;
                const int ntask = ngrp * nseg;
                // VALU time of the busiest wave per plane (columns + the window fill of every segment) against the useful columns
                const double wave_cols = (double)cdiv(ntask, 4) * (sl + 0.5);
                const double useful = (double)p.Hit * p.Wit / ((double)tiles_h * tiles_w);        // outputs of an average tile
                const double valu_eff = useful / (wave_cols * 4.0 * 8.0);
                const double stage_eff = (double)th * tw / ((double)ra * ca);                      // halo re-reads (L2 -> LDS)
                const double sweep = (double)p.T * wave_cols;
                const double startup = sweep / (sweep + 10.0);                                      // weights + ring fill per workgroup
                const double blocks = (double)p.N * tiles_h * tiles_w * p.nchunks;
                const double fill = blocks >= 512.0 ? blocks / (cdiv((int64_t)blocks, 512) * 512.0) : blocks / 512.0;
                const double score = valu_eff * (0.5 + 0.5 * stage_eff) * startup * (0.5 + 0.5 * fill);
                if (score > best) {
                    best = score;
                    p.TH = th; p.TW = tw; p.tiles_h = tiles_h; p.tiles_w = tiles_w;
                    p.RA = ra; p.CA = ca; p.RP = rp; p.slotb = slotb; p.vpt = cdiv(slotb, 4096);
                    p.ngrp = ngrp; p.nseg = nseg; p.SL = sl;
                }
            }
        }
    }
    if (best <= 0.0) return false;
    p.fdRP = make_fastdiv(p.RP); p.fdSeg = make_fastdiv(p.nseg);
    const int64_t per_n_a = (int64_t)p.T * p.Ha * p.Wa + p.cls;
    if ((int64_t)p.Ha * p.Wa * d->ldy >= (1ll << 31) || per_n_a * d->ldy >= (1ll << 40)) return false;
    return true;
}
// Rotating-accumulator form of the sweep (sf_dwsweep.h: sf_dwrot_kernel): forward, stride-1 data gradient, weight gradient.
// A tile is ngrp groups of 4 rows x nseg runs of SL columns, one (group, run) per wave.
// strides >= 3 (windows do not overlap): forward and weight gradient on sf_dwrot_kernel<., 3, ...> (packed staging), data
// gradient on sf_dwgap_dgrad_kernel
static bool dwgap_shape_ok(const sf_dw_desc* d) {
    if (d->kT != 3 || d->kH != 3 || d->kW != 3 || d->pT != 1 || d->pH != 1 || d->pW != 1) return false;
    if (d->sT != 1 || d->sH != d->sW || d->sH < 3 || d->To != d->Ti) return false;
    return d->C % 8 == 0 && d->Cw % 8 == 0;
}
static bool dwrot_plan(const sf_dw_desc* d, int dir, DwSweepParams& p, int& kmode, int& ks, int& ksl) {
    if (test_hook("SF_DW_SWEEP", 1) == 0) return false;
    const bool gap = dwgap_shape_ok(d);
    if (!dwsweep_shape_ok(d) && !gap) return false;
    if (dir == 1 && d->sH != 1) return false;           // stride 2: sf_dwsweep_kernel<1, 2>; strides >= 3: sf_dwgap_dgrad_kernel
    memset(&p, 0, sizeof(p));
    p.N = d->N; p.C = d->C; p.Cw = d->Cw; p.Cwreal = d->Cwreal ? d->Cwreal : d->Cw; p.cls = d->cls ? 1 : 0; p.T = d->Ti;
    p.nchunks = cdiv(d->C, 32);
    const int s = gap ? 3 : d->sH;                      // kernel template stride (3 = packed staging of a stride p.gs >= 3)
    p.gs = d->sH;
    if (dir == 0) { kmode = 0; ks = s; p.Ha = d->Hi; p.Wa = d->Wi; p.Hd = d->Ho; p.Wd = d->Wo; p.Hit = d->Ho; p.Wit = d->Wo; }
    else if (dir == 1) { kmode = 0; ks = 1; p.flip = 1; p.Ha = d->Ho; p.Wa = d->Wo; p.Hd = d->Hi; p.Wd = d->Wi; p.Hit = d->Hi; p.Wit = d->Wi; }
    else { kmode = 2; ks = s; p.Ha = d->Hi; p.Wa = d->Wi; p.Hb = d->Ho; p.Wb = d->Wo; p.Hit = d->Ho; p.Wit = d->Wo; }
    const int lds_cap = ks == 1 ? DwrLds<0, 1>::bytes : DwrLds<0, 2>::bytes;
    const int64_t max_rows = gap ? (int64_t)d->N * d->Ho * d->Wo : dwsweep_max_rows(d);
    const int f_sl = test_hook("SF_DWR_SL", 0), f_grp = test_hook("SF_DWR_NGRP", 0), f_seg = test_hook("SF_DWR_NSEG", 0);  // tests / tuning
    const int f_nr = test_hook("SF_DWR_NR", 0);
    double best = 0.0;
    static const int kSL[2] = {7, 4};
    for (int si = 0; si < 2; ++si) {
        const int sl = kSL[si];
        if (f_sl > 0 && sl != f_sl) continue;
        for (int ngrp = 1; ngrp <= 4; ++ngrp)
            for (int nseg = 1; ngrp * nseg <= 4; ++nseg) {
                if ((f_grp > 0 && ngrp != f_grp) || (f_seg > 0 && nseg != f_seg)) continue;
                const int th = 4 * ngrp, tw = sl * nseg;
                const int ca = (tw - 1) * ks + 3, ra = (th - 1) * ks + 3;
                int rp = ca * 64;
                if (ks != 2) { if (rp % 128 == 0) rp += 64; } else rp += 32;      // (stride * pitch) % 128 == 64: the rows of a read group
                const int slotb = roundup(ra * rp, 1024);
                if (slotb > SF_DWS_MAXVPT * 4096) continue;
                int rpb = 0, slotbB = 0;
                if (kmode == 2) {
                    rpb = tw * 64;
                    if (rpb % 128 == 0) rpb += 64;
                    slotbB = roundup(th * rpb, 1024);
                    if (slotbB > SF_DWS_MAXVPTB * 4096) continue;
                }
                // ring depth: up to three planes in flight when the LDS class holds them (measured: 3 / 4 / 5 slots within 3 % of each
                // other at the MViT stage-3 planes, profiles/r6_v10_ring_depth.txt -- the sweep is not bound by the copies' latency)
                int nr = f_nr > 0 ? f_nr : 4;
                while (nr >= 3 && nr * slotb + (nr - 1) * slotbB > lds_cap) --nr;
                if (nr < 3 || nr > SF_DWR_MAXNR) continue;
                if (nr > p.T + 1) nr = p.T + 1 > 3 ? p.T + 1 : 3;
                const int tiles_h = cdiv(p.Hit, th), tiles_w = cdiv(p.Wit, tw);
                if ((int64_t)p.N * tiles_h * tiles_w > max_rows) continue;
                const int ntask = ngrp * nseg;
                const double valu_eff = (double)p.Hit * p.Wit / ((double)tiles_h * tiles_w * ntask * 4.0 * sl);
                const double stage_eff = gap ? 1.0 : (double)(th * ks) * (tw * ks) / ((double)ra * ca);
                const double occ = ntask == 4 ? 1.0 : ntask == 3 ? 0.85 : ntask == 2 ? 0.7 : 0.5;     // idle waves hold registers and LDS
                const double run = (sl + 2.0 / ks) / (sl + 2.0);                                    // window words per output
                const double score = valu_eff * occ * (0.6 + 0.4 * stage_eff) * (0.9 + 0.1 * run);
                if (score > best) {
                    best = score;
                    ksl = sl;
                    p.nr = nr;
                    p.TH = th; p.TW = tw; p.tiles_h = tiles_h; p.tiles_w = tiles_w;
                    p.RA = ra; p.CA = ca; p.RP = rp; p.slotb = slotb; p.vpt = cdiv(slotb, 4096);
                    p.RB = th; p.CBt = tw; p.RPB = rpb; p.slotbB = slotbB; p.vptB = slotbB ? cdiv(slotbB, 4096) : 0;
                    p.ngrp = ngrp; p.nseg = nseg; p.SL = sl;
                }
            }
    }
    if (best <= 0.0) return false;
    p.fdRP = make_fastdiv(p.RP); p.fdRPB = make_fastdiv(p.RPB ? p.RPB : 1); p.fdSeg = make_fastdiv(p.nseg);
    const int64_t per_n_a = (int64_t)p.T * p.Ha * p.Wa + p.cls;
    const int lda = dir == 1 ? d->ldy : d->ldx;
    if ((int64_t)p.Ha * p.Wa * lda >= (1ll << 31) || per_n_a * lda >= (1ll << 40)) return false;
    if (kmode == 2 && (int64_t)p.Hb * p.Wb * d->ldy >= (1ll << 31)) return false;
    return true;
}
static void dwrot_launch(DwSweepParams& p, int kmode, int ks, int sl, bool stats, hipStream_t s) {
    const dim3 grid((unsigned)(p.N * p.tiles_h * p.tiles_w * p.nchunks));
    if (sf_trace()) fprintf(stderr, "[sfamd] dwrot: mode %d s=%d SL=%d N=%d C=%d T=%d a %dx%d it %dx%d TH=%d TW=%d tiles %dx%d RA=%d CA=%d RP=%d slot %d "
                       "(b %d) ring %d grp=%d seg=%d blocks=%u\n", kmode, ks, sl, p.N, p.C, p.T, p.Ha, p.Wa, p.Hit, p.Wit, p.TH, p.TW, p.tiles_h, p.tiles_w,
                       p.RA, p.CA, p.RP, p.slotb, p.slotbB, p.nr, p.ngrp, p.nseg, grid.x);
#define SF_DWR_LAUNCH(M, S, L, ST) hipLaunchKernelGGL((sf_dwrot_kernel<M, S, L, ST>), grid, dim3(SF_THREADS), 0, s, p)
#define SF_DWR_SL(M, S, ST) do { if (sl == 7) SF_DWR_LAUNCH(M, S, 7, ST); else SF_DWR_LAUNCH(M, S, 4, ST); } while (0)
    if (kmode == 0) {
        if (ks == 1) { if (stats) SF_DWR_SL(0, 1, true); else SF_DWR_SL(0, 1, false); }
        else if (ks == 2) { if (stats) SF_DWR_SL(0, 2, true); else SF_DWR_SL(0, 2, false); }
        else { if (stats) SF_DWR_SL(0, 3, true); else SF_DWR_SL(0, 3, false); }
    } else if (ks == 1) SF_DWR_SL(2, 1, false);
    else if (ks == 2) SF_DWR_SL(2, 2, false);
    else SF_DWR_SL(2, 3, false);
#undef SF_DWR_SL
#undef SF_DWR_LAUNCH
}
static void dwsweep_launch(DwSweepParams& p, bool stats, hipStream_t s) {
    const dim3 grid((unsigned)(p.N * p.tiles_h * p.tiles_w * p.nchunks));
    if (sf_trace()) fprintf(stderr, "[sfamd] dwsweep: mode 1 s=2 N=%d C=%d T=%d a %dx%d it %dx%d TH=%d TW=%d tiles %dx%d RA=%d CA=%d RP=%d slot %d "
                       "(b %d) grp=%d seg=%d SL=%d blocks=%u\n", p.N, p.C, p.T, p.Ha, p.Wa, p.Hit, p.Wit, p.TH, p.TW, p.tiles_h, p.tiles_w,
                       p.RA, p.CA, p.RP, p.slotb, p.slotbB, p.ngrp, p.nseg, p.SL, grid.x);
    if (stats) hipLaunchKernelGGL((sf_dwsweep_kernel<1, 2, true>), grid, dim3(SF_THREADS), 0, s, p);
    else hipLaunchKernelGGL((sf_dwsweep_kernel<1, 2, false>), grid, dim3(SF_THREADS), 0, s, p);
}
// Data gradient at strides >= 3 (sf_dwgap_dgrad_kernel): one thread per (input position, 8 channels)
static bool dwgap_plan(const sf_dw_desc* d, DwGapParams& gp, int& blocks) {
    if (test_hook("SF_DW_SWEEP", 1) == 0 || !dwgap_shape_ok(d) || 27 * d->Cw > SF_DW_GAP_W) return false;
    memset(&gp, 0, sizeof(gp));
    gp.N = d->N; gp.C = d->C; gp.Cw = d->Cw; gp.Cwreal = d->Cwreal ? d->Cwreal : d->Cw; gp.cls = d->cls ? 1 : 0;
    gp.T = d->Ti; gp.Hi = d->Hi; gp.Wi = d->Wi; gp.Ho = d->Ho; gp.Wo = d->Wo; gp.s = d->sH;
    const int64_t Si = (int64_t)d->Ti * d->Hi * d->Wi + gp.cls;
    gp.rows = (int64_t)d->N * Si;
    const int64_t items = gp.rows * (d->C / 8);
    if (items >= (1ll << 31)) return false;             // the kernel splits (uint32_t)item with fd_divmod: exact below 2^31 (sf_common.h)
    gp.fdRow = make_fastdiv((uint32_t)Si); gp.fdW = make_fastdiv(d->Wi); gp.fdH = make_fastdiv(d->Hi);
    gp.fdS = make_fastdiv(d->sH); gp.fdG = make_fastdiv(d->C / 8);
    blocks = cdiv(items, SF_THREADS * 4);
    if (blocks > 4096) blocks = 4096;
    return true;
}

// Temporal depthwise convolution (kT, 1, 1) / stride 1 / padding kT / 2 (X3D stem): one register-window pass (sf_dwtemporal.h).
// SF_DW_TEMPORAL=0 keeps the W-blocked stencils (A/B runs, read per call).  dir: 0 forward, 1 data gradient, 2 weight gradient.
static bool dwtemp_plan(const sf_dw_desc* d, int dir, DwTempParams& p) {
    const char* lv = getenv("SF_DW_TEMPORAL");
    if (lv && atoi(lv) == 0) return false;
    if (d->kH != 1 || d->kW != 1 || (d->kT != 3 && d->kT != 5 && d->kT != 7) || d->pT != d->kT / 2 || d->pH != 0 || d->pW != 0) return false;
    if (d->sT != 1 || d->sH != 1 || d->sW != 1 || d->To != d->Ti || d->Ho != d->Hi || d->Wo != d->Wi || d->cls) return false;
    if (d->C % 8 != 0 || d->C / 8 > SF_THREADS) return false;
    const int64_t cols = (int64_t)d->N * d->Hi * d->Wi;
    if (cols >= (1ll << 31) || (int64_t)d->Hi * d->Wi * (d->ldx > d->ldy ? d->ldx : d->ldy) >= (1ll << 31)) return false;
    memset(&p, 0, sizeof(p));
    p.N = d->N; p.C = d->C; p.Cw = d->Cw; p.Cwreal = d->Cwreal ? d->Cwreal : d->Cw; p.T = d->Ti; p.HW = d->Hi * d->Wi;
    p.G = d->C / 8; p.PP = SF_THREADS / p.G; p.cols = (int)cols; p.flip = dir == 1 ? 1 : 0;
    const int64_t passes = cdiv(cols, (int64_t)p.PP);
    // workgroups = rows of the partial tables: at most 2048 (forward statistics, finalized without a fold stage) / 1024 (weight gradient)
    const int forced = test_hook("SF_DWTP_BLOCKS", 0);       // tests: several passes per workgroup on small shapes
    const int64_t max_blocks = forced > 0 ? forced : dir == 2 ? 1024 : 2048;
    p.iters = (int)cdiv(passes, max_blocks);
    p.fdHW = make_fastdiv(p.HW); p.fdG = make_fastdiv(p.G);
    return true;
}
static int dwtemp_blocks(const DwTempParams& p) { return (int)cdiv(cdiv((int64_t)p.cols, (int64_t)p.PP), (int64_t)p.iters); }
static void dwtemp_launch(DwTempParams& p, int kT, int dir, bool stats, hipStream_t s) {
    const dim3 grid((unsigned)dwtemp_blocks(p));
    if (sf_trace()) fprintf(stderr, "[sfamd] dwtemporal: dir %d kT=%d N=%d C=%d T=%d HW=%d PP=%d iters=%d blocks=%u\n", dir, kT, p.N, p.C, p.T, p.HW, p.PP, p.iters, grid.x);
#define SF_DWTP_LAUNCH(K) do {                                                                                                   \
        if (dir == 2) hipLaunchKernelGGL((sf_dwtemporal_kernel<K, 2, false>), grid, dim3(SF_THREADS), 0, s, p);                    \
        else if (stats) hipLaunchKernelGGL((sf_dwtemporal_kernel<K, 0, true>), grid, dim3(SF_THREADS), 0, s, p);                   \
        else hipLaunchKernelGGL((sf_dwtemporal_kernel<K, 0, false>), grid, dim3(SF_THREADS), 0, s, p);                             \
    } while (0)
    if (kT == 3) SF_DWTP_LAUNCH(3);
    else if (kT == 5) SF_DWTP_LAUNCH(5);
    else SF_DWTP_LAUNCH(7);
#undef SF_DWTP_LAUNCH
}

// ------------------------------------------------------------------------------------------------
// One plan per call: the family that runs a depthwise convolution, its filled parameters and the rows of its side table.  Every
// launcher and every size query (sf_dwconv_fwd_blocks, _fwd_sample_rows, _dgrad_sum_rows, _pair_ok) reads this one function, so
// the tables a caller allocates agree with what runs.  dir: 0 forward, 1 data gradient, 2 weight gradient.  side_table: the call
// writes the forward's BatchNorm partial sums / the data gradient's column sums.
// Precedence: temporal (kT, 1, 1) window; the plane sweeps (rotating form, the stride-2 data gradient, the gap data gradient at
// strides >= 3); the W-blocked stencils; the generic stencils.
enum DwFamily { DW_TEMPORAL, DW_ROT, DW_SWEEP, DW_GAP, DW_BLOCKED, DW_GENERIC };
struct DwPlan {
    DwFamily fam;
    int64_t rows;           // side table rows: [rows][2][C] sums (dir 0 / 1; 0: this family leaves no column sums), [rows][taps][C] (dir 2)
    DwParams p; dim3 grid; DwBlockIdx bi; int kind;     // stencils (kind: dw_blocked_kind, 0 = generic)
    DwTempParams tp;
    DwSweepParams sp; int km, ks, sl;                   // DW_ROT (kernel mode, template stride, run length) / DW_SWEEP
    DwGapParams gp; int gblocks;
};
static int dw_plan(DwPlan& pl, const sf_dw_desc* d, int dir, bool side_table) {
    static const int kMaxBlocks[3] = {kDwFwdBlocks, 8192, kDwWgradBlocks};      // stencil row blocks per direction
    if (fill_dw(pl.p, d, dir != 1, kMaxBlocks[dir], pl.grid)) return -1;
    pl.rows = 0;
    pl.kind = 0;
    if (dwtemp_plan(d, dir, pl.tp)) {
        pl.fam = DW_TEMPORAL;
        if (dir != 1) pl.rows = dwtemp_blocks(pl.tp);
        return 0;
    }
    // with BatchNorm sums a cls row keeps the forward on the stencils (the sums on the sweeps serve X3D, which has no cls row)
    if (!(dir == 0 && side_table && d->cls) && dwrot_plan(d, dir, pl.sp, pl.km, pl.ks, pl.sl)) pl.fam = DW_ROT;
    else if (dir == 1 && dwsweep_plan(d, pl.sp)) pl.fam = DW_SWEEP;
    else if (dir == 1 && dwgap_plan(d, pl.gp, pl.gblocks)) { pl.fam = DW_GAP; return 0; }
    else {
        pl.kind = dw_blocked_kind(d);
        pl.fam = pl.kind ? DW_BLOCKED : DW_GENERIC;
        if (pl.kind) dw_block_plan(pl.p, pl.bi, d, dir != 1, kMaxBlocks[dir], pl.grid);
        if (dir != 1) pl.rows = pl.grid.x;
        return 0;
    }
    pl.rows = (int64_t)pl.sp.N * pl.sp.tiles_h * pl.sp.tiles_w;     // one row per (sample, tile)
    return 0;
}
static void dw_sweep_launch(DwPlan& pl, bool stats, hipStream_t s) {
    if (pl.fam == DW_ROT) dwrot_launch(pl.sp, pl.km, pl.ks, pl.sl, stats, s);
    else dwsweep_launch(pl.sp, stats, s);
}
// sums the [nblk][taps][ldc] partial rows of a weight gradient into dw (ldc = 0: C)
static void dw_wgrad_finalize(const sf_dw_desc* d, const float* wpart, int nblk, int ldc, float* dw, float scale, int zero_first,
                              hipStream_t s) {
    DwFinalizeParams f;
    f.wpart = wpart; f.nblk = nblk; f.taps = d->kT * d->kH * d->kW; f.C = d->C; f.Cw = d->Cw; f.ldc = ldc;
    f.Cwreal = d->Cwreal ? d->Cwreal : d->Cw;
    f.dw = dw; f.scale = scale; f.accumulate = zero_first ? 0 : 1;
    hipLaunchKernelGGL(sf_dwconv_wgrad_finalize_kernel, dim3(cdiv(f.taps * d->Cw, 32)), dim3(SF_THREADS), 0, s, f);
}

// rows of sf_dwconv_fwd's statistics table
extern "C" int sf_dwconv_fwd_blocks(const sf_dw_desc* d) {
    DwPlan pl;
    if (dw_plan(pl, d, 0, true)) return -1;
    return (int)pl.rows;
}
// Rows of sf_dwconv_fwd's statistics table that belong to ONE sample when the table is sample-major (the plane sweeps write one
// row per (sample, tile): rows [n * r, (n + 1) * r) are sample n's), 0 when the kernel this geometry takes cuts its rows without
// regard to samples.  Lets a caller take per-sample channel sums (the SE squeeze, operators.py:38-45) from the table instead of
// from a pass over y.
extern "C" int sf_dwconv_fwd_sample_rows(const sf_dw_desc* d) {
    DwPlan pl;
    if (dw_plan(pl, d, 0, true)) return -1;
    return pl.fam == DW_ROT ? pl.sp.tiles_h * pl.sp.tiles_w : 0;
}
extern "C" int sf_dwconv_fwd(const sf_dw_desc* d, const void* x, const float* w, void* y, float* stat_part,
                             sf_stream_t stream) {
    DwPlan pl;
    if (dw_plan(pl, d, 0, stat_part != nullptr)) return -1;
    REQUIRE(x && w && y, "sf_dwconv_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (pl.fam == DW_TEMPORAL) {
        DwTempParams& tp = pl.tp;
        tp.a = (const f16*)x; tp.lda = d->ldx; tp.dst = (f16*)y; tp.ldd = d->ldy; tp.w = w; tp.part = stat_part;
        dwtemp_launch(tp, d->kT, 0, stat_part != nullptr, s);
        return check_launch("dwconv_fwd (temporal)");
    }
    if (pl.fam == DW_ROT) {
        DwSweepParams& sp = pl.sp;
        sp.a = (const f16*)x; sp.lda = d->ldx; sp.dst = (f16*)y; sp.ldd = d->ldy; sp.w = w; sp.part = stat_part;
        dw_sweep_launch(pl, stat_part != nullptr, s);
        return check_launch("dwconv_fwd (rot)");
    }
    DwParams& p = pl.p;
    p.x = (const f16*)x; p.ldx = d->ldx; p.w = w; p.y = (f16*)y; p.ldy = d->ldy; p.stat_part = stat_part;
    if (pl.kind) SF_DW_DISPATCH_WT(pl.kind, sf_dwconv_fwd_blocked_kernel, pl.grid, s, p, pl.bi);
    else if (p.kT * p.kH * p.kW * p.Cw <= SF_DW_SMALL_W) hipLaunchKernelGGL(sf_dwconv_fwd_kernel<SF_DW_SMALL_W>, pl.grid, dim3(SF_THREADS), 0, s, p);
    else hipLaunchKernelGGL(sf_dwconv_fwd_kernel<SF_DW_MAX_W>, pl.grid, dim3(SF_THREADS), 0, s, p);
    return check_launch("dwconv_fwd");
}
// rows of the optional column-sum table of sf_dwconv_dgrad_sums ([rows][2][C]: slot 0 = per-workgroup column sums of dx, the
// cls row included; slot 1 unspecified), 0 when the kernel this geometry takes cannot leave them
extern "C" int sf_dwconv_dgrad_sum_rows(const sf_dw_desc* d) {
    DwPlan pl;
    if (dw_plan(pl, d, 1, true)) return -1;
    return (int)pl.rows;
}
static int dwconv_dgrad_impl(const sf_dw_desc* d, const void* dy, const float* w, void* dx, float* sum_part, sf_stream_t stream) {
    DwPlan pl;
    if (dw_plan(pl, d, 1, sum_part != nullptr)) return -1;
    REQUIRE(!sum_part || pl.rows > 0, "sf_dwconv_dgrad_sums: this geometry leaves no column sums (sf_dwconv_dgrad_sum_rows == 0)");
    REQUIRE(dy && w && dx, "sf_dwconv_dgrad: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (pl.fam == DW_TEMPORAL) {
        DwTempParams& tp = pl.tp;
        tp.a = (const f16*)dy; tp.lda = d->ldy; tp.dst = (f16*)dx; tp.ldd = d->ldx; tp.w = w;
        dwtemp_launch(tp, d->kT, 1, false, s);
        return check_launch("dwconv_dgrad (temporal)");
    }
    if (pl.fam == DW_ROT || pl.fam == DW_SWEEP) {
        DwSweepParams& sp = pl.sp;
        sp.a = (const f16*)dy; sp.lda = d->ldy; sp.dst = (f16*)dx; sp.ldd = d->ldx; sp.w = w; sp.part = sum_part;
        dw_sweep_launch(pl, sum_part != nullptr, s);
        return check_launch(pl.fam == DW_ROT ? "dwconv_dgrad (rot)" : "dwconv_dgrad (sweep)");
    }
    if (pl.fam == DW_GAP) {
        DwGapParams& gp = pl.gp;
        gp.dy = (const f16*)dy; gp.lddy = d->ldy; gp.dx = (f16*)dx; gp.lddx = d->ldx; gp.w = w;
        hipLaunchKernelGGL(sf_dwgap_dgrad_kernel, dim3(pl.gblocks), dim3(SF_THREADS), 0, s, gp);
        return check_launch("dwconv_dgrad (gap)");
    }
    DwParams& p = pl.p;
    p.dy = (const f16*)dy; p.lddy = d->ldy; p.w = w; p.y = (f16*)dx; p.ldy = d->ldx;
    if (pl.kind) SF_DW_DISPATCH_WT(pl.kind, sf_dwconv_dgrad_blocked_kernel, pl.grid, s, p, pl.bi);
    else if (p.kT * p.kH * p.kW * p.Cw <= SF_DW_SMALL_W) hipLaunchKernelGGL(sf_dwconv_dgrad_kernel<SF_DW_SMALL_W>, pl.grid, dim3(SF_THREADS), 0, s, p);
    else hipLaunchKernelGGL(sf_dwconv_dgrad_kernel<SF_DW_MAX_W>, pl.grid, dim3(SF_THREADS), 0, s, p);
    return check_launch("dwconv_dgrad");
}
extern "C" int sf_dwconv_dgrad(const sf_dw_desc* d, const void* dy, const float* w, void* dx, sf_stream_t stream) {
    return dwconv_dgrad_impl(d, dy, w, dx, nullptr, stream);
}
// sf_dwconv_dgrad that also leaves the column sums of dx: MViT's qkv Linear takes its bias gradient (the column sums of d(qkv),
// attention.py:318-330) from the three pooling data gradients that write d(qkv) instead of from a pass over it
extern "C" int sf_dwconv_dgrad_sums(const sf_dw_desc* d, const void* dy, const float* w, void* dx, float* sum_part,
                                    sf_stream_t stream) {
    REQUIRE(sum_part, "sf_dwconv_dgrad_sums: null table");
    return dwconv_dgrad_impl(d, dy, w, dx, sum_part, stream);
}
// ------------------------------------------------------------------------------------------------
// PAIR entry points (round 6): two depthwise convolutions of ONE geometry on two tensors in ONE launch per direction -- MViT's
// pool_k and pool_v of a block (attention.py:227-266: same kernel / stride / padding, adjacent channel slices of qkv, separate
// weights).  At the stage-3 / 4 planes (14 -> 7, 7 x 7) a launch is 25-35 us of start-up and ramp around 8 planes of work; both
// tensors behind one start-up cost 1.45x one (tools/dw_bench.py: C = 768 against C = 384 at the same plane).  The descriptor
// describes ONE tensor; the plane sweeps (sf_dwsweep.h, PAIR mode) must take the geometry in all three directions and C must be a
// multiple of 32: sf_dwconv_pair_ok.  Same arithmetic as two single calls, bit for bit.
extern "C" int sf_dwconv_pair_ok(const sf_dw_desc* d) {
    DwPlan pl;
    if (dw_plan(pl, d, 0, false)) return -1;
    if (test_hook("SF_DW_PAIR", 1) == 0 || d->C % 32 != 0) return 0;
    for (int dir = 0; dir < 3; ++dir)
        if ((dir > 0 && dw_plan(pl, d, dir, false)) || (pl.fam != DW_ROT && pl.fam != DW_SWEEP)) return 0;
    return 1;
}
static void dw_pair_plan(DwPlan& pl, const sf_dw_desc* d, int dir) {
    dw_plan(pl, d, dir, false);         // (taken: sf_dwconv_pair_ok)
    pl.sp.csplit = d->C; pl.sp.Cpart = 2 * d->C; pl.sp.nchunks *= 2;
}
extern "C" int sf_dwconv_fwd_pair(const sf_dw_desc* d, const void* x, const void* x2, const float* w, const float* w2, void* y,
                                  void* y2, sf_stream_t stream) {
    REQUIRE(sf_dwconv_pair_ok(d) == 1, "sf_dwconv_fwd_pair: geometry not taken (sf_dwconv_pair_ok)");
    REQUIRE(x && x2 && w && w2 && y && y2, "sf_dwconv_fwd_pair: null pointer");
    DwPlan pl;
    dw_pair_plan(pl, d, 0);
    DwSweepParams& sp = pl.sp;
    sp.a = (const f16*)x; sp.a2 = (const f16*)x2; sp.lda = d->ldx; sp.dst = (f16*)y; sp.dst2 = (f16*)y2; sp.ldd = d->ldy;
    sp.w = w; sp.w2 = w2;
    dw_sweep_launch(pl, false, (hipStream_t)stream);
    return check_launch("dwconv_fwd_pair");
}
extern "C" int sf_dwconv_dgrad_pair(const sf_dw_desc* d, const void* dy, const void* dy2, const float* w, const float* w2,
                                    void* dx, void* dx2, sf_stream_t stream) {
    REQUIRE(sf_dwconv_pair_ok(d) == 1, "sf_dwconv_dgrad_pair: geometry not taken (sf_dwconv_pair_ok)");
    REQUIRE(dy && dy2 && w && w2 && dx && dx2, "sf_dwconv_dgrad_pair: null pointer");
    DwPlan pl;
    dw_pair_plan(pl, d, 1);
    DwSweepParams& sp = pl.sp;
    sp.a = (const f16*)dy; sp.a2 = (const f16*)dy2; sp.lda = d->ldy; sp.dst = (f16*)dx; sp.dst2 = (f16*)dx2; sp.ldd = d->ldx;
    sp.w = w; sp.w2 = w2;
    dw_sweep_launch(pl, false, (hipStream_t)stream);
    return check_launch("dwconv_dgrad_pair");
}
// workspace: 2 x sf_dwconv_wgrad_workspace(d) bytes
extern "C" int sf_dwconv_wgrad_pair(const sf_dw_desc* d, const void* x, const void* x2, const void* dy, const void* dy2,
                                    float* dw, float* dw2, float out_scale, int zero_first, int zero_first2, void* workspace,
                                    int64_t workspace_bytes, sf_stream_t stream) {
    REQUIRE(sf_dwconv_pair_ok(d) == 1, "sf_dwconv_wgrad_pair: geometry not taken (sf_dwconv_pair_ok)");
    REQUIRE(x && x2 && dy && dy2 && dw && dw2 && workspace, "sf_dwconv_wgrad_pair: null pointer");
    DwPlan pl;
    dw_pair_plan(pl, d, 2);
    REQUIRE(workspace_bytes >= pl.rows * 27 * 2 * d->C * 4, "sf_dwconv_wgrad_pair: workspace too small");
    DwSweepParams& sp = pl.sp;
    sp.a = (const f16*)x; sp.a2 = (const f16*)x2; sp.lda = d->ldx; sp.b = (const f16*)dy; sp.b2 = (const f16*)dy2; sp.ldb = d->ldy;
    sp.part = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    dw_sweep_launch(pl, false, s);
    if (check_launch("dwconv_wgrad_pair")) return -1;
    dw_wgrad_finalize(d, (const float*)workspace, (int)pl.rows, 2 * d->C, dw, out_scale, zero_first, s);
    dw_wgrad_finalize(d, (const float*)workspace + d->C, (int)pl.rows, 2 * d->C, dw2, out_scale, zero_first2, s);
    return check_launch("dwconv_wgrad_pair_finalize");
}

// Partial-table bytes of sf_dwconv_wgrad: a bound over every family a call may take, whatever the per-call test hooks
// (SF_DW_SWEEP, SF_DW_TEMPORAL, SF_DWS_* / SF_DWR_* tilings) select -- callers cache the size per geometry.
extern "C" int64_t sf_dwconv_wgrad_workspace(const sf_dw_desc* d) {
    DwParams p;
    dim3 grid;
    if (fill_dw(p, d, true, kDwWgradBlocks, grid)) return -1;
    if (dw_blocked_kind(d)) {
        DwBlockIdx bi;
        dw_block_plan(p, bi, d, true, kDwWgradBlocks, grid);
    }
    int64_t rows = grid.x;                                                              // stencils
    if (dwsweep_shape_ok(d) && dwsweep_max_rows(d) > rows) rows = dwsweep_max_rows(d);  // rotating sweep, strides 1 / 2
    if (dwgap_shape_ok(d) && (int64_t)d->N * d->Ho * d->Wo > rows) rows = (int64_t)d->N * d->Ho * d->Wo;   // strides >= 3
    if (rows < 1024) rows = 1024;       // sf_dwtemporal_kernel: at most 1024 partial rows
    return rows * d->kT * d->kH * d->kW * d->C * 4;
}
extern "C" int sf_dwconv_wgrad(const sf_dw_desc* d, const void* x, const void* dy, float* dw, float out_scale,
                               int zero_first, void* workspace, int64_t workspace_bytes, sf_stream_t stream) {
    DwPlan pl;
    if (dw_plan(pl, d, 2, true)) return -1;
    REQUIRE(x && dy && dw && workspace, "sf_dwconv_wgrad: null pointer");
    const int taps = d->kT * d->kH * d->kW;
    REQUIRE(workspace_bytes >= pl.rows * taps * d->C * 4, "sf_dwconv_wgrad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (pl.fam == DW_TEMPORAL) {
        DwTempParams& tp = pl.tp;
        tp.a = (const f16*)x; tp.lda = d->ldx; tp.b = (const f16*)dy; tp.ldb = d->ldy; tp.part = (float*)workspace;
        dwtemp_launch(tp, d->kT, 2, false, s);
    } else if (pl.fam == DW_ROT) {
        DwSweepParams& sp = pl.sp;
        sp.a = (const f16*)x; sp.lda = d->ldx; sp.b = (const f16*)dy; sp.ldb = d->ldy; sp.part = (float*)workspace;
        dw_sweep_launch(pl, false, s);
    } else {
        REQUIRE(pl.grid.y == 1, "sf_dwconv_wgrad: C > 2048 is not supported");
        DwParams& p = pl.p;
        dim3 grid = pl.grid;
        p.x = (const f16*)x; p.ldx = d->ldx; p.dy = (const f16*)dy; p.lddy = d->ldy; p.wpart = (float*)workspace;
        grid.z = pl.kind ? d->kT : d->kT * cdiv(d->kH * d->kW, 9);
        if (pl.kind == 1) hipLaunchKernelGGL((sf_dwconv_wgrad_blocked_kernel<3, 1, SF_DW_SMALL_W>), grid, dim3(SF_THREADS), 0, s, p, pl.bi);
        else if (pl.kind == 2) hipLaunchKernelGGL((sf_dwconv_wgrad_blocked_kernel<3, 2, SF_DW_SMALL_W>), grid, dim3(SF_THREADS), 0, s, p, pl.bi);
        else if (pl.kind) hipLaunchKernelGGL((sf_dwconv_wgrad_blocked_kernel<1, 1, SF_DW_SMALL_W>), grid, dim3(SF_THREADS), 0, s, p, pl.bi);
        else hipLaunchKernelGGL(sf_dwconv_wgrad_kernel, grid, dim3(SF_THREADS), 0, s, p);
    }
    if (check_launch(pl.fam == DW_TEMPORAL ? "dwconv_wgrad (temporal)" : pl.fam == DW_ROT ? "dwconv_wgrad (rot)" : "dwconv_wgrad")) return -1;
    dw_wgrad_finalize(d, (const float*)workspace, (int)pl.rows, 0, dw, out_scale, zero_first, s);
    return check_launch("dwconv_wgrad_finalize");
}

// ---- relative-position terms + softmax of pooled attention
static int fill_relpos(RelPosParams& p, const sf_attn_desc* d) {
    REQUIRE(d != nullptr, "attention: null descriptor");
    REQUIRE(d->B > 0 && d->heads > 0 && d->D > 0 && d->D <= 128, "attention: bad shape (head dim <= 128)");
    REQUIRE(d->Nq == d->cls + d->qT * d->qH * d->qW && d->Nk == d->cls + d->kT * d->kH * d->kW,
            "attention: token counts do not match the (T,H,W) shapes");
    REQUIRE(d->kH + d->kW + d->kT <= 64, "attention: kH + kW + kT must be <= 64");
    memset(&p, 0, sizeof(p));
    p.B = d->B; p.Nq = d->Nq; p.heads = d->heads; p.D = d->D; p.cls = d->cls;
    p.qT = d->qT; p.qH = d->qH; p.qW = d->qW; p.KH = d->kH; p.KW = d->kW; p.KT = d->kT;
    p.rows_h = d->rows_h; p.rows_w = d->rows_w; p.rows_t = d->rows_t;
    p.fdHeads = make_fastdiv(d->heads); p.fdNq = make_fastdiv(d->Nq);
    p.fdW = make_fastdiv(d->qW); p.fdH = make_fastdiv(d->qH);
    return 0;
}
static int relpos_blocks(const sf_attn_desc* d) {
    const int64_t rows = (int64_t)d->B * d->Nq * d->heads;
    int blocks = cdiv(rows, 4);
    return blocks > 16384 ? 16384 : blocks;
}
extern "C" int sf_relpos_gather(const sf_attn_desc* d, const void* G, int32_t ldg, const int32_t* idx_h,
                                const int32_t* idx_w, const int32_t* idx_t, float* rq, sf_stream_t stream) {
    RelPosParams p;
    if (fill_relpos(p, d)) return -1;
    REQUIRE(G && idx_h && idx_w && idx_t && rq, "sf_relpos_gather: null pointer");
    REQUIRE(ldg >= d->rows_h + d->rows_w + d->rows_t, "sf_relpos_gather: pitch smaller than the table row count");
    p.idx_h = idx_h; p.idx_w = idx_w; p.idx_t = idx_t; p.rq = rq;
    const int R = d->kH + d->kW + d->kT;
    const int64_t total = (int64_t)d->B * d->Nq * d->heads * R;
    REQUIRE(total < (1ll << 31), "sf_relpos_gather: too many elements");
    if (ldg % 8 == 0 && ldg <= 256 && (uintptr_t)G % 16 == 0) {
        const int64_t rows = (int64_t)d->B * d->Nq * d->heads, chunks = (rows + 31) / 32;
        hipLaunchKernelGGL(sf_relpos_gather_lds_kernel, dim3((unsigned)(chunks < 8192 ? chunks : 8192)), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p, (const f16*)G, ldg, make_fastdiv((uint32_t)R), R, rows);
        return check_launch("relpos_gather");
    }
    hipLaunchKernelGGL(sf_relpos_gather_kernel, dim3(pool_grid(total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p,
                       (const f16*)G, ldg, make_fastdiv((uint32_t)R), total);
    return check_launch("relpos_gather");
}
extern "C" int sf_relpos_pack(const float* rel_h, const float* rel_w, const float* rel_t, int32_t rows_h, int32_t rows_w,
                              int32_t rows_t, int32_t D, int32_t TRp, void* t16, void* t16t, sf_stream_t stream) {
    REQUIRE(rel_h && rel_w && rel_t && t16 && t16t, "sf_relpos_pack: null pointer");
    REQUIRE(D > 0 && rows_h >= 0 && rows_w >= 0 && rows_t >= 0 && TRp >= rows_h + rows_w + rows_t && TRp % 8 == 0, "sf_relpos_pack: bad shape");
    RelPosTabParams p;
    memset(&p, 0, sizeof(p));
    p.tab[0] = rel_h; p.tab[1] = rel_w; p.tab[2] = rel_t; p.rows[0] = rows_h; p.rows[1] = rows_w; p.rows[2] = rows_t;
    p.D = D; p.TRp = TRp; p.t16 = (f16*)t16; p.t16t = (f16*)t16t;
    hipLaunchKernelGGL(sf_relpos_pack_kernel, dim3(pool_grid((int64_t)TRp * D)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("relpos_pack");
}
extern "C" int sf_relpos_unpack(const float* dtab, int32_t rows_h, int32_t rows_w, int32_t rows_t, int32_t D, float* grad_h,
                                float* grad_w, float* grad_t, int32_t acc_h, int32_t acc_w, int32_t acc_t, sf_stream_t stream) {
    REQUIRE(dtab && grad_h && grad_w && grad_t, "sf_relpos_unpack: null pointer");
    REQUIRE(D > 0 && rows_h >= 0 && rows_w >= 0 && rows_t >= 0 && rows_h + rows_w + rows_t > 0, "sf_relpos_unpack: bad shape");
    RelPosTabParams p;
    memset(&p, 0, sizeof(p));
    p.grad[0] = grad_h; p.grad[1] = grad_w; p.grad[2] = grad_t; p.rows[0] = rows_h; p.rows[1] = rows_w; p.rows[2] = rows_t;
    p.acc[0] = acc_h; p.acc[1] = acc_w; p.acc[2] = acc_t; p.D = D; p.dtab = dtab;
    hipLaunchKernelGGL(sf_relpos_unpack_kernel, dim3(pool_grid((int64_t)(rows_h + rows_w + rows_t) * D)), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("relpos_unpack");
}
extern "C" int sf_relpos_scatter(const sf_attn_desc* d, const float* drq, const int32_t* idx_h, const int32_t* idx_w,
                                 const int32_t* idx_t, void* E, int32_t lde, sf_stream_t stream) {
    RelPosParams p;
    if (fill_relpos(p, d)) return -1;
    REQUIRE(drq && idx_h && idx_w && idx_t && E, "sf_relpos_scatter: null pointer");
    REQUIRE(lde % 8 == 0 && lde >= d->rows_h + d->rows_w + d->rows_t, "sf_relpos_scatter: bad pitch");
    p.idx_h = idx_h; p.idx_w = idx_w; p.idx_t = idx_t; p.drq = drq;
    const int R = d->kH + d->kW + d->kT;
    const int64_t rows = (int64_t)d->B * d->Nq * d->heads, total = rows * R;
    REQUIRE(total < (1ll << 31), "sf_relpos_scatter: too many elements");
    REQUIRE((uintptr_t)E % 16 == 0, "sf_relpos_scatter: E must be 16-byte aligned");
    const int64_t chunks = (rows + SF_RELPOS_SC_ROWS - 1) / SF_RELPOS_SC_ROWS;
    if (lde <= SF_RELPOS_SC_LDE)
        hipLaunchKernelGGL(sf_relpos_scatter_lds_kernel, dim3((unsigned)(chunks < 8192 ? chunks : 8192)), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p, (f16*)E, lde, make_fastdiv((uint32_t)R), R, rows);
    else
        hipLaunchKernelGGL(sf_relpos_scatter_kernel, dim3((unsigned)(chunks < 8192 ? chunks : 8192)), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p, (f16*)E, lde, make_fastdiv((uint32_t)R), R, rows);
    return check_launch("relpos_scatter");
}
// out[i] (+)= scale * sum_b part[b*row_len + offset + i], i < n   (table gradients from per-block partials):
// 32 outputs per block x 8 segments of the block sum, fixed-order LDS fold
__global__ __launch_bounds__(SF_THREADS) void sf_rows_sum_kernel(const float* part, int nblk, int64_t row_len, int64_t offset,
                                                                  int n, float* out, float scale, int accumulate) {
    __shared__ double s_acc[8][32];
    const int ox = threadIdx.x & 31, seg = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + ox;
    double s = 0.0;
    if (i < n) {
        const float* src = part + offset + i;
        for (int b = seg; b < nblk; b += 8) s += (double)src[b * row_len];
    }
    s_acc[seg][ox] = s;
    __syncthreads();
    if (seg == 0 && i < n) {
        for (int k = 1; k < 8; ++k) s += s_acc[k][ox];
        const float v = (float)(s * scale);
        out[i] = accumulate ? out[i] + v : v;
    }
}
extern "C" int sf_rows_sum(const float* part, int32_t nblk, int64_t row_len, int64_t offset, int32_t n, float* out,
                           float scale, int accumulate, sf_stream_t stream) {
    REQUIRE(part && out && nblk > 0 && n > 0, "sf_rows_sum: bad arguments");
    hipLaunchKernelGGL(sf_rows_sum_kernel, dim3(cdiv(n, 32)), dim3(SF_THREADS), 0, (hipStream_t)stream, part, nblk,
                       row_len, offset, n, out, scale, accumulate);
    return check_launch("rows_sum");
}

static int fill_softmax(SoftmaxParams& p, const sf_attn_desc* d, void* s, int32_t lds, float scale) {
    REQUIRE(d != nullptr && s != nullptr, "softmax: null pointer");
    REQUIRE(lds % 8 == 0 && lds >= d->Nk && lds <= 64 * 8 * 4, "softmax: score pitch must be a multiple of 8 in [Nk, 2048]");
    memset(&p, 0, sizeof(p));
    p.s = (f16*)s; p.lds = lds; p.rows = d->B * d->heads * d->Nq;
    p.Nq = d->Nq; p.Nk = d->Nk; p.heads = d->heads; p.cls = d->cls; p.kT = d->kT; p.kH = d->kH; p.kW = d->kW;
    p.scale = scale; p.R = d->kH + d->kW + d->kT; p.KH = d->kH; p.KW = d->kW;
    p.fdNq = make_fastdiv(d->Nq); p.fdHeads = make_fastdiv(d->heads);
    p.fdkW = make_fastdiv(d->kW); p.fdkH = make_fastdiv(d->kH);
    return 0;
}
extern "C" int sf_softmax_fwd(const sf_attn_desc* d, void* s, int32_t lds, float scale, const float* rq, sf_stream_t stream) {
    SoftmaxParams p;
    if (fill_softmax(p, d, s, lds, scale)) return -1;
    // one lane per bias entry: the kernel stages a row's rq in s_rq[4][64]
    REQUIRE(!rq || p.R <= 64, "sf_softmax_fwd: kH + kW + kT must be <= 64 with a rel-pos bias");
    p.rq = rq;
    int blocks = cdiv(p.rows, 4);
    if (blocks > 16384) blocks = 16384;
    hipStream_t st = (hipStream_t)stream;
    if (lds <= 512) hipLaunchKernelGGL((sf_softmax_fwd_kernel<1>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    else if (lds <= 1024) hipLaunchKernelGGL((sf_softmax_fwd_kernel<2>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    else hipLaunchKernelGGL((sf_softmax_fwd_kernel<4>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    return check_launch("softmax_fwd");
}
extern "C" int sf_softmax_bwd(const sf_attn_desc* d, void* dp, const void* prob, int32_t lds, float scale, float* drq,
                              sf_stream_t stream) {
    SoftmaxParams p;
    if (fill_softmax(p, d, dp, lds, scale)) return -1;
    REQUIRE(prob != nullptr, "sf_softmax_bwd: null pointer");
    REQUIRE(!drq || p.R <= 64, "sf_softmax_bwd: kH + kW + kT must be <= 64 with a rel-pos bias");     // lane j < 64 owns drq[j]
    p.prob = (const f16*)prob; p.drq = drq;
    int blocks = cdiv(p.rows, 4);
    if (blocks > 16384) blocks = 16384;
    hipStream_t st = (hipStream_t)stream;
    if (lds <= 512) hipLaunchKernelGGL((sf_softmax_bwd_kernel<1>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    else if (lds <= 1024) hipLaunchKernelGGL((sf_softmax_bwd_kernel<2>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    else hipLaunchKernelGGL((sf_softmax_bwd_kernel<4>), dim3(blocks), dim3(SF_THREADS), 0, st, p);
    return check_launch("softmax_bwd");
}

// ------------------------------------------------------------------------------------------------
// fused attention (sf_attn.h)
// key tiles per wave of the key-side backward kernel: 2 (each Q / dO fragment read from LDS feeds two MFMAs) whenever the head has
// more than 64 keys and the accumulators of two tiles fit the register file (head dim <= 96); SF_ATTN_DKV_KT=1|2 forces one
static int attn_dkv_kt(const sf_attn_desc* d) {
    static const int kt_env = tune_knob("SF_ATTN_DKV_KT", 0);
    if (d->D > 96) return 1;
    if (kt_env == 1 || kt_env == 2) return kt_env;
    return d->Nk > 64 ? 2 : 1;
}
static int fill_attn(AttnParams& p, const sf_attn_desc* d, const char* who) {
    REQUIRE(d, "%s: null descriptor", who);
    REQUIRE(d->B > 0 && d->heads > 0 && d->Nq > 0 && d->Nk > 0, "%s: empty problem", who);
    REQUIRE(d->D % 32 == 0 && d->D >= 32 && d->D <= 128, "%s: head dim must be 32, 64, 96 or 128 (got %d)", who, d->D);
    REQUIRE(d->Nq == d->cls + d->qT * d->qH * d->qW && d->Nk == d->cls + d->kT * d->kH * d->kW, "%s: inconsistent descriptor", who);
    memset(&p, 0, sizeof(p));
    p.B = d->B; p.heads = d->heads; p.Nq = d->Nq; p.Nk = d->Nk; p.cls = d->cls;
    p.R = d->kH + d->kW + d->kT;
    p.qtiles = cdiv(d->Nq, 64); p.ktiles = cdiv(d->Nk, 64 * attn_dkv_kt(d));
    REQUIRE((int64_t)d->B * d->heads * (p.qtiles > p.ktiles ? p.qtiles : p.ktiles) < (1ll << 28), "%s: too many tiles", who);
    // dK/dV: split the queries so that ~1024 workgroups exist (Nk is small), at least 8 query chunks per split
    const int nchq = cdiv(d->Nq, 32);
    // SF_ATTN_DKV_WGS: workgroups the query split aims for.  512 = one round of resident workgroups: MViTv2-S needs no split
    // then -- no fp32 partial tables (154 MB per call), no reduce kernel; measured against 1024 (two rounds, rounds 1-3) on
    // the stage-3 shape: 314 vs 344 us for the whole backward call (profiles/r4/r4_v8_attn_ab.txt)
    static const int wgs_target = tune_knob("SF_ATTN_DKV_WGS", 512);
    int splits = cdiv(wgs_target > 0 ? wgs_target : 512, (int64_t)d->B * d->heads * p.ktiles);
    if (splits > nchq / 8) splits = nchq / 8;
    if (splits < 1) splits = 1;
    p.chunks_per_split = cdiv(nchq, splits);
    p.qsplits = cdiv(nchq, p.chunks_per_split);
    return 0;
}
// workspace of sf_attn_bwd: [fp32 split partials of dK / dV (qsplits > 1)] [rq hi / lo fp16 rows (relative positions)]
static int64_t attn_part_bytes(const AttnParams& p, const sf_attn_desc* d) {
    return p.qsplits > 1 ? (int64_t)p.qsplits * 2 * d->B * d->Nk * d->heads * d->D * 4 : 0;
}
static int64_t attn_ws_bytes(const AttnParams& p, const sf_attn_desc* d) {
    const bool rel = d->rows_h + d->rows_w + d->rows_t > 0;
    return attn_part_bytes(p, d) + (rel ? (int64_t)d->B * d->Nq * d->heads * 128 * 2 : 0);
}
// two 16-query column tiles per wave (halves the LDS operand traffic per MFMA) once there are enough workgroups;
// SF_ATTN_QT=1|2 forces either form
static bool attn_two_tiles(const sf_attn_desc* d) {
    static const int qt_env = tune_knob("SF_ATTN_QT", 0);
    return qt_env ? qt_env == 2 : (int64_t)d->B * d->heads * cdiv(d->Nq, 128) >= 1024;
}
#define SF_ATTN_LAUNCH_Q(KERNEL, D_, two, grid, st, p)                                                     \
    do {                                                                                                   \
        const int kd_ = (D_) / 32;                                                                         \
        if (two) {                                                                                         \
            if (kd_ == 1) hipLaunchKernelGGL((KERNEL<1, 2>), dim3(grid), dim3(SF_THREADS), 0, st, p);      \
            else if (kd_ == 2) hipLaunchKernelGGL((KERNEL<2, 2>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
            else if (kd_ == 3) hipLaunchKernelGGL((KERNEL<3, 2>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
            else hipLaunchKernelGGL((KERNEL<4, 2>), dim3(grid), dim3(SF_THREADS), 0, st, p);               \
        } else {                                                                                           \
            if (kd_ == 1) hipLaunchKernelGGL((KERNEL<1, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p);      \
            else if (kd_ == 2) hipLaunchKernelGGL((KERNEL<2, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
            else if (kd_ == 3) hipLaunchKernelGGL((KERNEL<3, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
            else hipLaunchKernelGGL((KERNEL<4, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p);               \
        }                                                                                                  \
    } while (0)
#define SF_ATTN_LAUNCH(KERNEL, D_, grid, st, p)                                                     \
    do {                                                                                            \
        switch ((D_) / 32) {                                                                        \
            case 1: hipLaunchKernelGGL((KERNEL<1>), dim3(grid), dim3(SF_THREADS), 0, st, p); break; \
            case 2: hipLaunchKernelGGL((KERNEL<2>), dim3(grid), dim3(SF_THREADS), 0, st, p); break; \
            case 3: hipLaunchKernelGGL((KERNEL<3>), dim3(grid), dim3(SF_THREADS), 0, st, p); break; \
            default: hipLaunchKernelGGL((KERNEL<4>), dim3(grid), dim3(SF_THREADS), 0, st, p); break; \
        }                                                                                           \
    } while (0)

extern "C" int sf_attn_fwd(const sf_attn_desc* d, const void* q, int32_t ldq, const void* k, const void* v, int32_t ldk,
                           float scale, const float* rq, const void* onehot, int32_t residual, void* o, int32_t ldo,
                           float* lse, sf_stream_t stream) {
    AttnParams p;
    if (fill_attn(p, d, "sf_attn_fwd")) return -1;
    REQUIRE(q && k && v && o && lse, "sf_attn_fwd: null pointer");
    REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 4 == 0, "sf_attn_fwd: row pitches must be multiples of 8");
    REQUIRE(ldk < (1 << 20), "sf_attn_fwd: ldk too large for the 27-bit chunk offsets");
    REQUIRE((rq == nullptr) == (onehot == nullptr), "sf_attn_fwd: rq and onehot come together");
    REQUIRE(!rq || p.R <= SF_ATTN_RMAX, "sf_attn_fwd: kH + kW + kT = %d exceeds %d", p.R, SF_ATTN_RMAX);
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.ldq = ldq; p.ldk = ldk;
    p.out = (f16*)o; p.ldout = ldo; p.rq = rq; p.oh = (const f16*)onehot; p.lse = lse;
    p.scale = scale; p.scale2 = scale * SF_LOG2E; p.residual = residual;
    if (!rq) p.R = 0;
    p.ablate = tune_knob("SF_ATTN_ABLATE", 0);        // diagnostic builds only (wrong results)
    const bool qt2 = attn_two_tiles(d);
    if (qt2) p.qtiles = cdiv(d->Nq, 128);
    {
        const int grid = d->B * d->heads * p.qtiles;
        hipStream_t st = (hipStream_t)stream;
#define SF_FWD(KD_, QT_)                                                                                                 \
    do {                                                                                                                 \
        if (p.R > 32) hipLaunchKernelGGL((sf_attn_fwd_kernel<KD_, QT_, true>), dim3(grid), dim3(SF_THREADS), 0, st, p);  \
        else hipLaunchKernelGGL((sf_attn_fwd_kernel<KD_, QT_, false>), dim3(grid), dim3(SF_THREADS), 0, st, p);          \
    } while (0)
        switch (d->D / 32 * 2 + (qt2 ? 1 : 0)) {
            case 2: SF_FWD(1, 1); break;
            case 3: SF_FWD(1, 2); break;
            case 4: SF_FWD(2, 1); break;
            case 5: SF_FWD(2, 2); break;
            case 6: SF_FWD(3, 1); break;
            case 7: SF_FWD(3, 2); break;
            case 8: SF_FWD(4, 1); break;
            default: SF_FWD(4, 2); break;
        }
#undef SF_FWD
    }
    return check_launch("attn_fwd");
}

extern "C" int64_t sf_attn_bwd_workspace(const sf_attn_desc* d) {
    AttnParams p;
    if (fill_attn(p, d, "sf_attn_bwd_workspace")) return -1;
    return attn_ws_bytes(p, d);
}

extern "C" int sf_attn_bwd(const sf_attn_desc* d, const void* q, int32_t ldq, const void* k, const void* v, int32_t ldk,
                           float scale, const float* rq, const void* onehot, int32_t residual, const void* o,
                           const void* dout, int32_t ldo, const float* lse, float* delta, void* dq, int32_t lddq, void* dk,
                           void* dv, int32_t lddk, float* drq, void* workspace, int64_t workspace_bytes,
                           sf_stream_t stream) {
    AttnParams p;
    if (fill_attn(p, d, "sf_attn_bwd")) return -1;
    REQUIRE(q && k && v && o && dout && lse && delta && dq && dk && dv, "sf_attn_bwd: null pointer");
    REQUIRE((rq == nullptr) == (drq == nullptr) && (rq == nullptr) == (onehot == nullptr),
            "sf_attn_bwd: rq, onehot and drq come together");
    REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 8 == 0 && lddq % 4 == 0 && lddk % 4 == 0, "sf_attn_bwd: bad row pitch");
    REQUIRE(ldq < (1 << 20) && ldk < (1 << 20) && ldo < (1 << 20) && d->heads < 8192, "sf_attn_bwd: row pitch too large for the 27-bit chunk offsets");
    REQUIRE(!rq || p.R <= SF_ATTN_RMAX, "sf_attn_bwd: kH + kW + kT = %d exceeds %d", p.R, SF_ATTN_RMAX);
    const int64_t need = attn_ws_bytes(p, d);
    REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "sf_attn_bwd: workspace too small (%lld < %lld bytes)",
            (long long)workspace_bytes, (long long)need);
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.ldq = ldq; p.ldk = ldk;
    p.o = (const f16*)o; p.dout = (const f16*)dout; p.ldo = ldo;
    p.out = (f16*)dq; p.ldout = lddq; p.dk = (f16*)dk; p.dv = (f16*)dv; p.lddk = lddk;
    p.rq = rq; p.drq = drq; p.oh = (const f16*)onehot; p.lse = const_cast<float*>(lse); p.delta = delta;
    p.scale = scale; p.scale2 = scale * SF_LOG2E; p.residual = residual; p.part = (float*)workspace;
    if (!rq) p.R = 0;
    if (rq) {
        REQUIRE(d->rows_h + d->rows_w + d->rows_t > 0, "sf_attn_bwd: rq given but the descriptor has no relative-position tables");
        p.rqs = (f16*)((char*)workspace + attn_part_bytes(p, d));
    }
    hipStream_t st = (hipStream_t)stream;
    {
        static const int dq_qt = tune_knob("SF_ATTN_DQ_QT", 0);       // 1 | 2 forces the query-side backward alone (A/B)
        const bool qt2 = dq_qt ? dq_qt == 2 : attn_two_tiles(d);
        const int qtiles = qt2 ? cdiv(d->Nq, 128) : p.qtiles;
        AttnParams pq = p;
        pq.qtiles = qtiles;
        SF_ATTN_LAUNCH_Q(sf_attn_bwd_dq_kernel, d->D, qt2, d->B * d->heads * qtiles, st, pq);   // also writes delta
    }
    if (check_launch("attn_bwd_dq")) return -1;
    {
        // waves per SIMD the key-side kernel is compiled for: 2 (no spills; 508 vs 505 clips/s, profiles/r1_visit14_*) or 3
        static const int occ = tune_knob("SF_ATTN_DKV_OCC", 2);
        const int grid = d->B * d->heads * p.ktiles * p.qsplits;
        const int kd = d->D / 32;
        const int kt = attn_dkv_kt(d);
        p.ablate = tune_knob("SF_ATTN_ABLATE", 0);        // diagnostic builds only (wrong results)
#define SF_DKV(KD_)                                                                                              \
    do {                                                                                                         \
        if (kt == 2 && p.R <= 32) hipLaunchKernelGGL((sf_attn_bwd_dkv_kernel<KD_, 2, 2, false>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
        else if (kt == 2) hipLaunchKernelGGL((sf_attn_bwd_dkv_kernel<KD_, 2, 2>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
        else if (occ == 2) hipLaunchKernelGGL((sf_attn_bwd_dkv_kernel<KD_, 2, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p); \
        else hipLaunchKernelGGL((sf_attn_bwd_dkv_kernel<KD_, 3, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p);   \
    } while (0)
        if (kd == 1) SF_DKV(1); else if (kd == 2) SF_DKV(2); else if (kd == 3) SF_DKV(3);
        else hipLaunchKernelGGL((sf_attn_bwd_dkv_kernel<4, 2, 1>), dim3(grid), dim3(SF_THREADS), 0, st, p);
#undef SF_DKV
    }
    if (check_launch("attn_bwd_dkv")) return -1;
    if (p.qsplits > 1) {
        AttnReduceParams r;
        r.part = p.part; r.qsplits = p.qsplits; r.C = d->heads * d->D; r.slab = (int64_t)d->B * d->Nk * r.C;
        r.dk = p.dk; r.dv = p.dv; r.lddk = lddk; r.scale = scale; r.fdC4 = make_fastdiv(r.C / 4);
        hipLaunchKernelGGL(sf_attn_reduce_kernel, dim3(pool_grid(r.slab / 2)), dim3(SF_THREADS), 0, st, r);
        return check_launch("attn_reduce");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// RoI head (sf_roi.h)
static int fill_tmean(TMeanParams& p, int32_t B, int32_t T, int64_t HW, int32_t C, const char* who) {
    REQUIRE(B > 0 && T > 0 && HW > 0 && C > 0 && C % 8 == 0, "%s: bad shape", who);
    memset(&p, 0, sizeof(p));
    p.T = T; p.C = C; p.HW = HW;
    p.total = (int64_t)B * HW * (C / 8);
    REQUIRE(p.total < (1ll << 31) && (int64_t)B * HW < (1ll << 31), "%s: too many elements", who);
    p.fdG = make_fastdiv(C / 8); p.fdHW = make_fastdiv((uint32_t)HW);
    return 0;
}
extern "C" int sf_tmean_fwd(int32_t B, int32_t T, int64_t HW, int32_t C, const void* x, int32_t ldx, float* m,
                            sf_stream_t stream) {
    TMeanParams p;
    if (fill_tmean(p, B, T, HW, C, "sf_tmean_fwd")) return -1;
    REQUIRE(x && m && ldx % 8 == 0 && ldx >= C, "sf_tmean_fwd: bad arguments");
    p.x = (const f16*)x; p.ldx = ldx; p.m = m;
    hipLaunchKernelGGL(sf_tmean_fwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("tmean_fwd");
}
extern "C" int sf_tmean_bwd(int32_t B, int32_t T, int64_t HW, int32_t C, const float* dm, void* dx, int32_t lddx,
                            sf_stream_t stream) {
    TMeanParams p;
    if (fill_tmean(p, B, T, HW, C, "sf_tmean_bwd")) return -1;
    REQUIRE(dm && dx && lddx % 8 == 0 && lddx >= C, "sf_tmean_bwd: bad arguments");
    p.dm = dm; p.dx = (f16*)dx; p.lddx = lddx;
    hipLaunchKernelGGL(sf_tmean_bwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("tmean_bwd");
}
static int fill_roi(RoiParams& p, int32_t R, int32_t B, int32_t H, int32_t W, int32_t C, int32_t res, float scale,
                    int32_t aligned, const float* rois, const char* who) {
    REQUIRE(R > 0 && B > 0 && H > 0 && W > 0 && C > 0 && rois, "%s: bad arguments", who);
    REQUIRE(res >= 1 && res * res <= 255, "%s: resolution must satisfy res*res <= 255 (got %d)", who, res);
    memset(&p, 0, sizeof(p));
    p.R = R; p.B = B; p.H = H; p.W = W; p.C = C; p.res = res; p.scale = scale; p.aligned = aligned; p.rois = rois;
    return 0;
}
extern "C" int sf_roi_align_max_fwd(int32_t R, int32_t B, int32_t H, int32_t W, int32_t C, int32_t res, float scale,
                                    int32_t aligned, const float* m, const float* rois, float* out, int32_t ldo,
                                    int32_t col0, void* argmax, sf_stream_t stream) {
    RoiParams p;
    if (fill_roi(p, R, B, H, W, C, res, scale, aligned, rois, "sf_roi_align_max_fwd")) return -1;
    REQUIRE(m && out && argmax && col0 >= 0 && col0 + C <= ldo, "sf_roi_align_max_fwd: bad output placement");
    p.m = m; p.out = out; p.ldo = ldo; p.col0 = col0; p.arg = (unsigned char*)argmax;
    hipLaunchKernelGGL(sf_roi_align_max_fwd_kernel, dim3(cdiv((int64_t)R * C, SF_THREADS)), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("roi_align_max_fwd");
}
extern "C" int sf_roi_align_max_bwd(int32_t R, int32_t B, int32_t H, int32_t W, int32_t C, int32_t res, float scale,
                                    int32_t aligned, const float* rois, const float* dout, int32_t lddo, int32_t col0,
                                    const void* argmax, float* dm, sf_stream_t stream) {
    RoiParams p;
    if (fill_roi(p, R, B, H, W, C, res, scale, aligned, rois, "sf_roi_align_max_bwd")) return -1;
    REQUIRE(dout && argmax && dm && col0 >= 0 && col0 + C <= lddo, "sf_roi_align_max_bwd: bad arguments");
    p.dout = dout; p.lddo = lddo; p.col0 = col0; p.arg = (unsigned char*)const_cast<void*>(argmax); p.dm = dm;
    hipLaunchKernelGGL(sf_roi_align_max_bwd_kernel, dim3(cdiv((int64_t)R * C, SF_THREADS)), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("roi_align_max_bwd");
}

// ================================================================================================
// MixUp / CutMix of the batch (sf_mixup.h; replaces mixup_fn(inputs[0], labels), tools/train_net.py:109-111).  Kernel
// launches only, scalars by value: they run eagerly between two replays and write the step's static buffers.
static const int kMixBlocks = 2048;         // 256 CUs x 8 resident blocks; the rest of the clip is grid-strided
static int mix_grid_x(int64_t items, int rows) {
    int64_t b = (items + SF_THREADS - 1) / SF_THREADS;
    const int64_t cap = kMixBlocks / rows > 0 ? kMixBlocks / rows : 1;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
static int check_mix_box(const char* who, int32_t mode, int32_t H, int32_t W, int32_t yl, int32_t yh, int32_t xl, int32_t xh) {
    REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (mixup) or 1 (cutmix)", who);
    REQUIRE(mode == 0 || (0 <= yl && yl <= yh && yh <= H && 0 <= xl && xl <= xh && xh <= W),
            "%s: box rows [%d, %d) columns [%d, %d) outside the %d x %d plane", who, yl, yh, xl, xh, H, W);
    return 0;
}
extern "C" int sf_mix_clip_f32(const float* src, float* dst, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                               int32_t mode, float lam, float one_minus_lam, int32_t yl, int32_t yh, int32_t xl, int32_t xh,
                               sf_stream_t stream) {
    REQUIRE(src && dst, "sf_mix_clip_f32: null pointer");
    REQUIRE(B > 0 && B < 65536 && C > 0 && T > 0 && H > 0 && W > 0, "sf_mix_clip_f32: bad shape");
    if (check_mix_box("sf_mix_clip_f32", mode, H, W, yl, yh, xl, xh)) return -1;
    MixClipParams p;
    memset(&p, 0, sizeof(p));
    p.S = (int64_t)C * T * H * W;
    REQUIRE(p.S < (1ll << 31), "sf_mix_clip_f32: more than 2^31 elements per sample");
    REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, "sf_mix_clip_f32: buffers must be 4-byte aligned");
    const bool inplace = (const float*)dst == src;
    REQUIRE(inplace || dst + (int64_t)B * p.S <= src || src + (int64_t)B * p.S <= dst,
            "sf_mix_clip_f32: dst must be src (in place) or must not overlap it");
    p.src = src; p.dst = dst; p.B = B; p.H = H; p.W = W; p.lam = lam; p.oml = one_minus_lam;
    p.yl = yl; p.yh = yh; p.xl = xl; p.xh = xh;
    const bool aligned = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && p.S % 4 == 0;
    const int64_t planes = (int64_t)C * T;
    if (mode == 0) {
        const int pairs = (B + 1) / 2;
        const int64_t n = aligned ? p.S / 4 : p.S;
        dim3 grid(mix_grid_x(n, pairs), pairs);
        if (aligned) hipLaunchKernelGGL(sf_mixup_clip_kernel<4>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(sf_mixup_clip_kernel<1>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
        return check_launch("mix_clip_f32 (mixup)");
    }
    p.vec_ok = aligned && W % 4 == 0;
    if (inplace) {
        const int pairs = B / 2;                            // the middle sample of an odd batch is left as it is
        if (yl == yh || xl == xh || pairs == 0) return 0;   // empty box: nothing to swap
        p.g0 = xl / 4;
        const int ngroups = (xh - 1) / 4 - p.g0 + 1;
        p.fdG = make_fastdiv((uint32_t)ngroups); p.fdR = make_fastdiv((uint32_t)(yh - yl));
        p.items = planes * (yh - yl) * ngroups;
        hipLaunchKernelGGL(sf_cutmix_swap_kernel, dim3(mix_grid_x(p.items, pairs), pairs), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p);
        return check_launch("mix_clip_f32 (cutmix)");
    }
    const int ngroups = (W + 3) / 4;
    p.fdG = make_fastdiv((uint32_t)ngroups); p.fdR = make_fastdiv((uint32_t)H);
    p.items = planes * H * ngroups;
    hipLaunchKernelGGL(sf_cutmix_copy_kernel, dim3(mix_grid_x(p.items, B), B), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("mix_clip_f32 (cutmix copy)");
}
extern "C" int sf_mix_targets(const int64_t* labels, int32_t B, int32_t K, float on_value, float off_value, float lam,
                              float one_minus_lam, float* out, sf_stream_t stream) {
    REQUIRE(labels && out, "sf_mix_targets: null pointer");
    REQUIRE(B > 0 && K > 0 && (int64_t)B * K < (1ll << 31), "sf_mix_targets: bad shape");
    MixTargetsParams p;
    p.labels = labels; p.B = B; p.K = K; p.on = on_value; p.off = off_value; p.lam = lam; p.oml = one_minus_lam; p.out = out;
    p.total = (int64_t)B * K;
    p.fdK = make_fastdiv((uint32_t)K);
    hipLaunchKernelGGL(sf_mix_targets_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("mix_targets");
}

// ================================================================================================
// Random erasing of the batch (sf_erase.h; replaces RandomErasing.__call__ on the host clip, datasets/kinetics.py:437-447).
// The draw arrives as one table (layout: sf_erase.h); the HOST copy is validated and sizes the grid, the kernels read the
// device copy.  Kernel launches only.
static int check_erase_table(const char* who, const int32_t* th, int32_t nrows, int32_t words, int32_t mode, int32_t N,
                             int32_t C, int32_t T, int32_t H, int32_t W, int64_t* max_items) {
    REQUIRE(mode == SF_ERASE_CONST || mode == SF_ERASE_RAND || mode == SF_ERASE_PIXEL,
            "%s: erase mode must be 0 (const), 1 (rand) or 2 (pixel)", who);
    REQUIRE(th && nrows >= 0 && nrows < 65536, "%s: null erase table or more than 65535 rows", who);
    const int64_t head = (int64_t)nrows * SF_ERASE_ROW_WORDS + N + 1;
    REQUIRE(words >= head, "%s: erase table of %d words is shorter than %d rows + %d + 1 sample offsets", who, words, nrows, N);
    const int32_t* first = th + (int64_t)nrows * SF_ERASE_ROW_WORDS;
    REQUIRE(first[0] == 0 && first[N] == nrows, "%s: erase table sample offsets must run from 0 to the row count", who);
    int64_t most = 0;
    for (int n = 0; n < N; ++n) {
        REQUIRE(first[n] <= first[n + 1], "%s: erase table sample offsets must ascend", who);
        for (int r = first[n]; r < first[n + 1]; ++r) {
            const int32_t* p = th + (int64_t)r * SF_ERASE_ROW_WORDS;
            REQUIRE(p[0] == n && p[10] == first[n + 1], "%s: erase row %d is not filed under its sample", who, r);
            REQUIRE(0 <= p[1] && p[1] <= p[2] && p[2] <= T && p[3] >= 0 && p[5] >= 0 && p[3] <= H - p[5] && p[4] >= 0 && p[6] >= 0
                    && p[4] <= W - p[6],
                    "%s: erase row %d (frames [%d, %d), rows [%d, %d), columns [%d, %d)) lies outside the %d x %d x %d clip", who,
                    r, p[1], p[2], p[3], p[3] + p[5], p[4], p[4] + p[6], T, H, W);
            if (mode == SF_ERASE_RAND)
                REQUIRE(p[9] >= head && (int64_t)p[9] + (int64_t)(p[2] - p[1]) * C <= words,
                        "%s: colours of erase row %d lie outside the table", who, r);
            const int64_t items = (int64_t)C * (p[2] - p[1]) * p[5] * ((p[6] + 2) / 4 + 1);
            if (p[6] > 0 && items > most) most = items;
        }
    }
    *max_items = most;
    return 0;
}
extern "C" int sf_erase_clip_f32(const float* src, float* dst, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W,
                                 int32_t mode, const int32_t* table_host, const int32_t* table_dev, int32_t nrows,
                                 int32_t table_words, sf_stream_t stream) {
    REQUIRE(src && dst && table_dev, "sf_erase_clip_f32: null pointer");
    REQUIRE(N > 0 && N < 65536 && C > 0 && T > 0 && H > 0 && W > 0, "sf_erase_clip_f32: bad shape");
    EraseClipParams p;
    memset(&p, 0, sizeof(p));
    p.S = (int64_t)C * T * H * W;
    REQUIRE(p.S < (1ll << 30), "sf_erase_clip_f32: more than 2^30 elements per sample");
    REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, "sf_erase_clip_f32: buffers must be 4-byte aligned");
    const bool inplace = (const float*)dst == src;
    REQUIRE(inplace || dst + (int64_t)N * p.S <= src || src + (int64_t)N * p.S <= dst,
            "sf_erase_clip_f32: dst must be src (in place) or must not overlap it");
    int64_t most = 0;
    if (check_erase_table("sf_erase_clip_f32", table_host, nrows, table_words, mode, N, C, T, H, W, &most)) return -1;
    p.src = src; p.dst = dst; p.tab = table_dev; p.first_row = table_dev + (int64_t)nrows * SF_ERASE_ROW_WORDS;
    p.N = N; p.C = C; p.T = T; p.H = H; p.W = W; p.mode = mode;
    if (inplace) {
        if (most == 0) return 0;                            // nothing to erase: nothing is launched
        hipLaunchKernelGGL(sf_erase_inplace_kernel, dim3(mix_grid_x(most, nrows), nrows), dim3(SF_THREADS), 0,
                           (hipStream_t)stream, p);
        return check_launch("erase_clip_f32");
    }
    p.items = (p.S + 3) / 4;
    hipLaunchKernelGGL(sf_erase_copy_kernel, dim3(mix_grid_x(p.items, N), N), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("erase_clip_f32 (copy)");
}
// ================================================================================================
// Spatial sampling of the batch (sf_sample.h; replaces utils.spatial_sampling on the normalised host clip,
// datasets/kinetics.py:410-435).  The draw arrives as one table with a row per sample (layout: sf_sample.h); the HOST copy is
// validated, the kernels read the device copy.  Kernel launches only.
static int check_crop_table(const char* who, const int32_t* th, int32_t N, int32_t Hs, int32_t Ws, int32_t S) {
    REQUIRE(th, "%s: null crop table", who);
    // (float)r must be exact and (win + i) * Ws * 3 stays far inside int64; the limit is what the coordinate rule assumes
    REQUIRE(Hs > 0 && Ws > 0 && Hs < (1 << 16) && Ws < (1 << 16) && S > 0 && S < (1 << 16),
            "%s: frame %d x %d / crop %d must be positive and below 65536", who, Hs, Ws, S);
    for (int n = 0; n < N; ++n) {
        const int32_t* c = th + (int64_t)n * SF_CROP_ROW_WORDS;
        REQUIRE(c[0] > 0 && c[0] <= Hs && c[1] > 0 && c[1] <= Ws,
                "%s: crop row %d: valid size %d x %d is not inside the %d x %d buffer", who, n, c[0], c[1], Hs, Ws);
        REQUIRE(c[4] > 0 && c[5] > 0 && c[2] >= 0 && c[3] >= 0 && c[2] <= c[0] - c[4] && c[3] <= c[1] - c[5],
                "%s: crop row %d: window rows [%d, %d) columns [%d, %d) lies outside the valid %d x %d", who, n, c[2],
                c[2] + c[4], c[3], c[3] + c[5], c[0], c[1]);
        REQUIRE(c[6] > 0 && c[7] > 0 && c[6] < (1 << 16) && c[7] < (1 << 16),
                "%s: crop row %d: resized size %d x %d must be positive and below 65536", who, n, c[6], c[7]);
        REQUIRE(c[8] >= 0 && c[9] >= 0 && c[8] <= c[6] - S && c[9] <= c[7] - S,
                "%s: crop row %d: crop %d at (%d, %d) lies outside the resized %d x %d", who, n, S, c[8], c[9], c[6], c[7]);
        REQUIRE(c[10] == 0 || c[10] == 1, "%s: crop row %d: flip must be 0 or 1", who, n);
    }
    return 0;
}
// what every kernel that reads uint8 frames through pack_clip_norm needs: the source, the (n, t, row, column) index space of
// Ho x Wo output planes and the normalisation
static void fill_pack_clip(PackClipParams& p, const void* frames, int32_t N, int32_t Tin, int32_t Tout, int32_t Ho, int32_t Wo,
                           float mean0, float mean1, float mean2, float std0, float std1, float std2) {
    const int64_t HW = (int64_t)Ho * Wo;
    p.frames = (const unsigned char*)frames; p.N = N; p.Tin = Tin; p.Tout = Tout; p.HW = HW;
    p.mean[0] = mean0; p.mean[1] = mean1; p.mean[2] = mean2; p.stdv[0] = std0; p.stdv[1] = std1; p.stdv[2] = std2;
    p.total = (int64_t)N * Tout * HW;
    p.fdHW = make_fastdiv((uint32_t)HW); p.fdT = make_fastdiv((uint32_t)Tout); p.fdW = make_fastdiv((uint32_t)Wo);
}
static void fill_sample_geom(SampleGeom& g, const int32_t* crop_dev, int32_t Hs, int32_t Ws, int32_t S) {
    g.crop = crop_dev; g.Hs = Hs; g.Ws = Ws; g.S = S;
}
extern "C" int sf_sample_clip_u8(const void* frames, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* crop_host,
                                 const int32_t* crop_dev, int32_t S, float mean0, float mean1, float mean2, float std0,
                                 float std1, float std2, float* out, sf_stream_t stream) {
    REQUIRE(frames && out && crop_dev, "sf_sample_clip_u8: null pointer");
    REQUIRE(N > 0 && T > 0, "sf_sample_clip_u8: bad shape");
    REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "sf_sample_clip_u8: zero std");
    REQUIRE((uintptr_t)out % 4 == 0, "sf_sample_clip_u8: out must be 4-byte aligned");
    if (check_crop_table("sf_sample_clip_u8", crop_host, N, Hs, Ws, S)) return -1;
    SampleClipParams m;
    memset(&m, 0, sizeof(m));
    PackClipParams& p = m.k;
    fill_pack_clip(p, frames, N, T, T, S, S, mean0, mean1, mean2, std0, std1, std2);
    REQUIRE(p.total < (1ll << 31) && (int64_t)N * T * Hs * Ws < (1ll << 40), "sf_sample_clip_u8: too many pixels");
    fill_sample_geom(p.g, crop_dev, Hs, Ws, S);
    m.dst = out;
    hipLaunchKernelGGL(sf_sample_clip_u8_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, m);
    return check_launch("sample_clip_u8");
}

// ================================================================================================
// The packed path (sf_pack.h): decoded uint8 frames -> the stems' W-pair buffer, one launch per pathway, with the batch's input
// stages between the pixel and the rounding.  One launcher behind the four entry points; what an entry point's argument list
// does not carry arrives as a null stage.  Kernel launches only.
struct PackCrop { const int32_t* host; const int32_t* dev; int32_t S; };
struct PackErase { int32_t mode; const int32_t* host; const int32_t* dev; int32_t nrows, words; };
struct PackMix { int32_t mode; float lam, oml; int32_t yl, yh, xl, xh; };
// H x W: the frames (with a crop: the padded source buffer, and the output plane is S x S).  The entry points with an erase
// stage take mix mode -1 (no mixing); sf_pack_clip_u8_mix always mixes.
static int pack_clip_impl(const char* who, const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index,
                          int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2, int32_t reverse,
                          void* out, const PackCrop* crop, const PackErase* erase, const PackMix* mix, sf_stream_t stream) {
    REQUIRE(frames && out && (!crop || crop->dev), "%s: null pointer", who);
    if (crop) {
        REQUIRE(N > 0 && Tin > 0 && Tout > 0, "%s: bad shape", who);
        REQUIRE(crop->S > 0 && crop->S % 2 == 0, "%s: the crop size must be even (W pairs)", who);
    } else {
        REQUIRE(N > 0 && Tin > 0 && Tout > 0 && H > 0 && W > 0 && W % 2 == 0, "%s: bad shape (W must be even)", who);
    }
    REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "%s: zero std", who);
    const int32_t Ho = crop ? crop->S : H, Wo = crop ? crop->S : W;     // the output plane: erase table and cutmix box live in it
    const bool mixing = mix && !(erase && mix->mode == -1);
    if (mix && erase) REQUIRE(mix->mode >= -1 && mix->mode <= 1, "%s: mix mode must be -1 (none), 0 (mixup) or 1 (cutmix)", who);
    if (crop && check_crop_table(who, crop->host, N, H, W, crop->S)) return -1;
    if (mixing && check_mix_box(who, mix->mode, Ho, Wo, mix->yl, mix->yh, mix->xl, mix->xh)) return -1;
    int64_t most = 0;
    if (erase) {
        REQUIRE((erase->host == nullptr) == (erase->dev == nullptr), "%s: the erase table needs both of its copies", who);
        if (erase->host && check_erase_table(who, erase->host, erase->nrows, erase->words, erase->mode, N, 3, Tin, Ho, Wo, &most))
            return -1;
    }
    PackClipParams p;
    memset(&p, 0, sizeof(p));
    fill_pack_clip(p, frames, N, Tin, Tout, Ho, Wo, mean0, mean1, mean2, std0, std1, std2);
    REQUIRE(p.total < (1ll << 31) && (int64_t)N * Tin * H * W < (1ll << 40), "%s: too many pixels", who);
    p.t_index = t_index; p.reverse = reverse; p.out = (f16*)out;
    p.mix = mixing ? mix->mode : -1;
    if (mixing) { p.lam = mix->lam; p.oml = mix->oml; }
    if (p.mix == 1) { p.yl = mix->yl; p.yh = mix->yh; p.xl = mix->xl; p.xh = mix->xh; }
    if (erase && erase->dev && erase->nrows > 0) {
        p.erase_mode = erase->mode;
        p.tab = erase->dev;
        p.first_row = erase->dev + (int64_t)erase->nrows * SF_ERASE_ROW_WORDS;
    }
    if (crop) fill_sample_geom(p.g, crop->dev, H, W, crop->S);
    const dim3 grid(pool_grid(p.total)), block(SF_THREADS);
    if (crop) hipLaunchKernelGGL((sf_pack_clip_kernel<PackSampled, true, true>), grid, block, 0, (hipStream_t)stream, p);
    else if (erase) hipLaunchKernelGGL((sf_pack_clip_kernel<PackDirect, true, true>), grid, block, 0, (hipStream_t)stream, p);
    else if (mix) hipLaunchKernelGGL((sf_pack_clip_kernel<PackDirect, false, true>), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((sf_pack_clip_kernel<PackDirect, false, false>), grid, block, 0, (hipStream_t)stream, p);
    return check_launch(who + 3);           // "pack_clip_u8..."
}
extern "C" int sf_pack_clip_u8(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index,
                               int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                               int32_t reverse, void* out, sf_stream_t stream) {
    return pack_clip_impl("sf_pack_clip_u8", frames, N, Tin, H, W, t_index, Tout, mean0, mean1, mean2, std0, std1, std2, reverse, out,
                          nullptr, nullptr, nullptr, stream);
}
extern "C" int sf_pack_clip_u8_mix(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index,
                                   int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                   int32_t reverse, void* out, int32_t mode, float lam, float one_minus_lam, int32_t yl,
                                   int32_t yh, int32_t xl, int32_t xh, sf_stream_t stream) {
    const PackMix mix = {mode, lam, one_minus_lam, yl, yh, xl, xh};
    return pack_clip_impl("sf_pack_clip_u8_mix", frames, N, Tin, H, W, t_index, Tout, mean0, mean1, mean2, std0, std1, std2, reverse,
                          out, nullptr, nullptr, &mix, stream);
}
extern "C" int sf_pack_clip_u8_aug(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index,
                                   int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                   int32_t reverse, void* out, int32_t erase_mode, const int32_t* table_host,
                                   const int32_t* table_dev, int32_t nrows, int32_t table_words, int32_t mix_mode, float lam,
                                   float one_minus_lam, int32_t yl, int32_t yh, int32_t xl, int32_t xh, sf_stream_t stream) {
    const PackErase erase = {erase_mode, table_host, table_dev, nrows, table_words};
    const PackMix mix = {mix_mode, lam, one_minus_lam, yl, yh, xl, xh};
    return pack_clip_impl("sf_pack_clip_u8_aug", frames, N, Tin, H, W, t_index, Tout, mean0, mean1, mean2, std0, std1, std2, reverse,
                          out, nullptr, &erase, &mix, stream);
}
extern "C" int sf_pack_clip_u8_sample(const void* frames, int32_t N, int32_t Tin, int32_t Hs, int32_t Ws, const int32_t* t_index,
                                      int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                      int32_t reverse, void* out, const int32_t* crop_host, const int32_t* crop_dev, int32_t S,
                                      int32_t erase_mode, const int32_t* table_host, const int32_t* table_dev, int32_t nrows,
                                      int32_t table_words, int32_t mix_mode, float lam, float one_minus_lam, int32_t yl,
                                      int32_t yh, int32_t xl, int32_t xh, sf_stream_t stream) {
    const PackCrop crop = {crop_host, crop_dev, S};
    const PackErase erase = {erase_mode, table_host, table_dev, nrows, table_words};
    const PackMix mix = {mix_mode, lam, one_minus_lam, yl, yh, xl, xh};
    return pack_clip_impl("sf_pack_clip_u8_sample", frames, N, Tin, Hs, Ws, t_index, Tout, mean0, mean1, mean2, std0, std1, std2,
                          reverse, out, &crop, &erase, &mix, stream);
}

// ================================================================================================
// Colour augmentation of the AVA batch (sf_color.h; replaces transform.color_jitter / lighting_jitter / color_normalization and
// the channel reordering on the host clip, datasets/ava_dataset.py:306-333).  The draw arrives as one table with a row per sample
// (layout: sf_color.h); the HOST copy is validated and decides what is launched, the kernels read the device copy.  Kernel
// launches only.
extern "C" int sf_color_chunks(int64_t HW) {
    REQUIRE(HW > 0 && HW <= (int64_t)SF_COLOR_CHUNK * SF_COLOR_MAX_CHUNKS, "sf_color_chunks: a frame must have 1 .. %d pixels",
            SF_COLOR_CHUNK * SF_COLOR_MAX_CHUNKS);
    return (int)((HW + SF_COLOR_CHUNK - 1) / SF_COLOR_CHUNK);
}
extern "C" int sf_color_sum_depth(void) { return SF_COLOR_SUM_DEPTH; }
// returns the number of rows with a contrast slot, -1 for a bad table
static int check_color_table(const char* who, const int32_t* th, int32_t N) {
    REQUIRE(th, "%s: null colour table", who);
    int contrast = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t* w = th + (int64_t)n * SF_COLOR_ROW_WORDS;
        int seen = 0;
        for (int s = 0; s < 3; ++s) {
            REQUIRE(w[s] >= -1 && w[s] <= 2, "%s: colour row %d: op %d of slot %d is none of -1, 0, 1, 2", who, n, w[s], s);
            if (w[s] < 0) continue;
            REQUIRE(!(seen >> w[s] & 1), "%s: colour row %d: op %d appears twice", who, n, w[s]);
            seen |= 1 << w[s];
        }
        for (int k = 4; k < 13; ++k)                        // an exponent of all ones: infinity or NaN
            REQUIRE((w[k] & 0x7f800000) != 0x7f800000, "%s: colour row %d: word %d is not a finite float", who, n, k);
        contrast += seen >> 1 & 1;
    }
    return contrast;
}
static int fill_color_params(const char* who, ColorParams& p, const float* clip, int32_t N, int32_t T, int64_t HW,
                             const int32_t* table_dev, bool& vec) {
    REQUIRE(clip && table_dev, "%s: null pointer", who);
    REQUIRE(N > 0 && T > 0 && (int64_t)N * T <= 65535, "%s: bad shape (N * T must be 1 .. 65535)", who);
    REQUIRE(HW > 0 && HW <= (int64_t)SF_COLOR_CHUNK * SF_COLOR_MAX_CHUNKS, "%s: a frame must have 1 .. %d pixels", who,
            SF_COLOR_CHUNK * SF_COLOR_MAX_CHUNKS);
    REQUIRE((int64_t)N * T * HW < (1ll << 31), "%s: too many pixels", who);
    REQUIRE((uintptr_t)clip % 4 == 0, "%s: the clip must be 4-byte aligned", who);
    memset(&p, 0, sizeof(p));
    p.clip = const_cast<float*>(clip); p.table = table_dev; p.N = N; p.T = T; p.HW = HW;
    p.chunks = (int)((HW + SF_COLOR_CHUNK - 1) / SF_COLOR_CHUNK);
    vec = (uintptr_t)clip % 16 == 0 && HW % 4 == 0;         // every (n, c, t) plane then starts on a 16-byte boundary
    return 0;
}
extern "C" int sf_color_frame_means_f32(const float* clip, int32_t N, int32_t T, int64_t HW, const int32_t* table_host,
                                        const int32_t* table_dev, float* partials, float* means, sf_stream_t stream) {
    ColorParams p;
    bool vec;
    if (fill_color_params("sf_color_frame_means_f32", p, clip, N, T, HW, table_dev, vec)) return -1;
    REQUIRE(partials && means, "sf_color_frame_means_f32: null pointer");
    const int contrast = check_color_table("sf_color_frame_means_f32", table_host, N);
    if (contrast < 0) return -1;
    if (contrast == 0) return 0;                            // nothing to reduce: nothing is launched
    p.partials = partials; p.means = means;
    const dim3 grid(p.chunks, N * T);
    if (vec) hipLaunchKernelGGL(sf_color_frame_sums_kernel<4>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(sf_color_frame_sums_kernel<1>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    if (check_launch("color_frame_sums")) return -1;
    hipLaunchKernelGGL(sf_color_frame_means_kernel, dim3(cdiv(N * T, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("color_frame_means");
}
extern "C" int sf_color_clip_f32(float* clip, int32_t N, int32_t T, int64_t HW, const int32_t* table_host,
                                 const int32_t* table_dev, const float* means, float mean0, float mean1, float mean2, float std0,
                                 float std1, float std2, int32_t reverse, sf_stream_t stream) {
    ColorParams p;
    bool vec;
    if (fill_color_params("sf_color_clip_f32", p, clip, N, T, HW, table_dev, vec)) return -1;
    REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "sf_color_clip_f32: zero std");
    const int contrast = check_color_table("sf_color_clip_f32", table_host, N);
    if (contrast < 0) return -1;
    REQUIRE(contrast == 0 || means, "sf_color_clip_f32: a row with contrast needs the frame means");
    p.means = const_cast<float*>(means);
    p.mean[0] = mean0; p.mean[1] = mean1; p.mean[2] = mean2; p.stdv[0] = std0; p.stdv[1] = std1; p.stdv[2] = std2;
    p.reverse = reverse;
    const int V = vec ? 4 : 1;
    p.total = (int64_t)N * T * (HW / V);
    p.fdG = make_fastdiv((uint32_t)(HW / V)); p.fdT = make_fastdiv((uint32_t)T);
    if (vec) hipLaunchKernelGGL(sf_color_clip_kernel<4>, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(sf_color_clip_kernel<1>, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("color_clip_f32");
}

// ================================================================================================
// The dense uint8 frame buffer (sf_u8frames.h) of the two stages below: its geometry, the choice of u8_walk's arm, a row's valid size.
template <class P>
static int fill_u8_frames(const char* who, P& p, const void* src, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_dev) {
    REQUIRE(src && table_dev, "%s: null pointer", who);
    REQUIRE(N > 0 && T > 0 && (int64_t)N * T <= 65535, "%s: bad shape (N * T must be 1 .. 65535)", who);
    REQUIRE(Hs > 0 && Ws > 0 && Hs < (1 << 16) && Ws < (1 << 16) && (int64_t)Hs * Ws * 3 < (1ll << 31),
            "%s: a frame of %d x %d is empty or has 2^31 bytes or more", who, Hs, Ws);
    memset(&p, 0, sizeof(p));
    p.src = (const unsigned char*)src; p.table = table_dev; p.N = N; p.T = T; p.Hs = Hs; p.Ws = Ws; p.slab = Hs * Ws;
    p.fdW = make_fastdiv((uint32_t)Ws);
    return 0;
}
// u8_walk's 16-byte arm: every frame slab starts on a 16-byte boundary in src and in dst (null: a pass that stores nothing)
static int u8_frames_vec(const void* src, const void* dst, int slab) {
    return (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && slab % SF_U8_PIX == 0;
}
static int check_valid_size(const char* who, int n, int32_t h, int32_t w, int32_t Hs, int32_t Ws) {
    REQUIRE(h > 0 && h <= Hs && w > 0 && w <= Ws, "%s: row %d: valid size %d x %d is not inside the %d x %d buffer", who, n, h, w, Hs, Ws);
    return 0;
}

// ================================================================================================
// RandAugment of the batch (sf_randaug.h; replaces the PIL loop of rand_augment_transform on the decoded frames,
// datasets/kinetics.py:389-400).  One call is one LAYER of the draw: a table with a row per sample (layout: sf_randaug.h); the
// HOST copy is validated and decides what is launched, the kernels read the device copy.  Kernel launches only.
extern "C" int sf_randaug_chunk(void) { return SF_U8_CHUNK; }
// counts the rows that need a histogram / a lookup table; -1 for a bad table
static int check_randaug_table(const char* who, const int32_t* th, int32_t N, int32_t Hs, int32_t Ws, int& hist_rows, int& lut_rows) {
    REQUIRE(th, "%s: null table", who);
    hist_rows = lut_rows = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t* w = th + (int64_t)n * SF_RANDAUG_ROW_WORDS;
        const int cls = w[0], op = w[1];
        REQUIRE(op >= 0 && op < SF_RANDAUG_OPS, "%s: row %d: unknown op code %d", who, n, op);
        REQUIRE(cls >= 0 && cls <= 4, "%s: row %d: unknown class %d", who, n, cls);
        const bool is_lut = op == 0 || op == 1 || op == 2 || op == 4 || op == 5 || op == 6 || op == 8 || op == 9;
        const bool is_affine = op == 3 || op == 11 || op == 12 || op == 13 || op == 14;
        REQUIRE(cls == 0 || (cls == 1 && is_lut) || (cls == 2 && op == 7) || (cls == 3 && op == 10) || (cls == 4 && is_affine),
                "%s: row %d: op %d is not of class %d", who, n, op, cls);
        if (check_valid_size(who, n, w[5], w[6], Hs, Ws)) return -1;
        if (cls == 0) continue;
        REQUIRE(op != 4 || (w[2] >= 0 && w[2] <= 8), "%s: row %d: Posterize keeps 0 .. 8 bits (got %d)", who, n, w[2]);
        REQUIRE(op != 5 || (w[2] >= 0 && w[2] <= 256), "%s: row %d: Solarize takes a threshold of 0 .. 256 (got %d)", who, n, w[2]);
        REQUIRE(op != 6 || (w[2] >= 0 && w[2] <= 255), "%s: row %d: SolarizeAdd adds 0 .. 255 (got %d)", who, n, w[2]);
        REQUIRE((w[3] & 0x7f800000) != 0x7f800000, "%s: row %d: the blend factor is not a finite float", who, n);
        if (cls == 4) {
            REQUIRE(w[4] == 0 || w[4] == 1, "%s: row %d: filter %d is neither 0 (bilinear) nor 1 (bicubic)", who, n, w[4]);
            for (int k = 0; k < 6; ++k)                     // an exponent of all ones: infinity or NaN
                REQUIRE((w[9 + 2 * k] & 0x7ff00000) != 0x7ff00000, "%s: row %d: matrix entry %d is not finite", who, n, k);
        }
        lut_rows += cls == 1;
        hist_rows += randaug_needs_hist(cls, op);
    }
    return 0;
}
extern "C" int sf_randaug_hist_u8(const void* src, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                                  const int32_t* table_dev, int32_t* hist, sf_stream_t stream) {
    RandAugParams p;
    if (fill_u8_frames("sf_randaug_hist_u8", p, src, N, T, Hs, Ws, table_dev)) return -1;
    int hist_rows, lut_rows;
    if (check_randaug_table("sf_randaug_hist_u8", table_host, N, Hs, Ws, hist_rows, lut_rows)) return -1;
    if (hist_rows == 0) return 0;                           // nothing to count: nothing is launched
    REQUIRE(hist && (uintptr_t)hist % 4 == 0, "sf_randaug_hist_u8: hist must be a 4-byte aligned pointer");
    p.hist = hist;
    p.vec = u8_frames_vec(src, nullptr, p.slab);
    hipLaunchKernelGGL(sf_randaug_hist_zero_kernel, dim3(N * T), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    if (check_launch("randaug_hist_zero")) return -1;
    hipLaunchKernelGGL(sf_randaug_hist_kernel, dim3(cdiv(p.slab, SF_U8_CHUNK), N * T), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("randaug_hist");
}
extern "C" int sf_randaug_layer_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws,
                                   const int32_t* table_host, const int32_t* table_dev, const int32_t* hist, void* lut,
                                   sf_stream_t stream) {
    RandAugParams p;
    if (fill_u8_frames("sf_randaug_layer_u8", p, src, N, T, Hs, Ws, table_dev)) return -1;
    REQUIRE(dst && dst != src, "sf_randaug_layer_u8: dst must be another buffer than src");
    int hist_rows, lut_rows;
    if (check_randaug_table("sf_randaug_layer_u8", table_host, N, Hs, Ws, hist_rows, lut_rows)) return -1;
    REQUIRE(hist_rows == 0 || hist, "sf_randaug_layer_u8: a row with AutoContrast, Equalize or Contrast needs the histograms");
    REQUIRE(lut_rows == 0 || lut, "sf_randaug_layer_u8: a row with a table op needs the table scratch");
    p.dst = (unsigned char*)dst; p.hist = const_cast<int32_t*>(hist); p.lut = (unsigned char*)lut;
    p.vec = u8_frames_vec(src, dst, p.slab);
    if (lut_rows) {
        hipLaunchKernelGGL(sf_randaug_lut_kernel, dim3(N * T), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
        if (check_launch("randaug_lut")) return -1;
    }
    hipLaunchKernelGGL(sf_randaug_stream_kernel, dim3(cdiv(p.slab, SF_U8_CHUNK), N * T), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("randaug_stream");
}

// ================================================================================================
// SSL colour augmentation of the batch (sf_sslcolor.h; replaces transform.color_jitter_video_ssl on the decoded frames,
// datasets/kinetics.py:378-387).  One table with a row per clip (layout: sf_sslcolor.h); the HOST copy is validated and decides
// what is launched, the kernels read the device copy.  Kernel launches only.
// counts the rows that need the histogram / the streaming pass / the blur; -1 for a bad table
static int check_sslcolor_table(const char* who, const int32_t* th, int32_t N, int32_t Hs, int32_t Ws, int& hist_rows,
                                int& stream_rows, int& blur_rows) {
    REQUIRE(th, "%s: null table", who);
    hist_rows = stream_rows = blur_rows = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t* w = th + (int64_t)n * SF_SSLCOLOR_ROW_WORDS;
        const int flags = w[0], order = w[1];
        REQUIRE(flags >= 0 && flags < 16, "%s: row %d: unknown flags %d", who, n, flags);
        if (check_valid_size(who, n, w[9], w[10], Hs, Ws)) return -1;
        if (flags & SF_SSLCOLOR_JITTER) {
            REQUIRE(order >= 0 && order < (1 << 16), "%s: row %d: the op order has more than four fields", who, n);
            int seen = 0;
            for (int k = 0; k < 4; ++k) {
                const int op = (order >> (4 * k)) & 15;
                if (op == SF_SSLCOLOR_NOP) continue;
                REQUIRE(op < 4, "%s: row %d: unknown op code %d", who, n, op);
                REQUIRE(!(seen & (1 << op)), "%s: row %d: op %d is drawn twice", who, n, op);
                seen |= 1 << op;
            }
            for (int k = 2; k <= 4; ++k)
                REQUIRE((w[k] & 0x7f800000) != 0x7f800000, "%s: row %d: blend factor %d is not a finite float", who, n, k - 2);
            REQUIRE(w[5] >= 0 && w[5] <= 255, "%s: row %d: the hue shift is 0 .. 255 (got %d)", who, n, w[5]);
        }
        if (flags & SF_SSLCOLOR_BLUR) {
            REQUIRE(w[6] >= 0 && 3 * (w[6] + 1) <= SF_SSLCOLOR_HALO, "%s: row %d: box radius %d is not 0 or 1 (sigma <= 2)", who, n, w[6]);
            REQUIRE(w[7] > 0 && w[8] >= 0 && (int64_t)(2 * w[6] + 1) * w[7] + 2 * (int64_t)w[8] <= (1 << 24),
                    "%s: row %d: the box weights do not sum to 2^24 or less", who, n);
        }
        hist_rows += sslcolor_needs_hist(flags, order);
        stream_rows += (flags & (SF_SSLCOLOR_JITTER | SF_SSLCOLOR_GREY)) != 0;
        blur_rows += (flags & SF_SSLCOLOR_BLUR) != 0;
    }
    return 0;
}
extern "C" int sf_sslcolor_hist_u8(const void* src, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                                   const int32_t* table_dev, int32_t* hist, sf_stream_t stream) {
    SslColorParams p;
    if (fill_u8_frames("sf_sslcolor_hist_u8", p, src, N, T, Hs, Ws, table_dev)) return -1;
    int hist_rows, stream_rows, blur_rows;
    if (check_sslcolor_table("sf_sslcolor_hist_u8", table_host, N, Hs, Ws, hist_rows, stream_rows, blur_rows)) return -1;
    if (hist_rows == 0) return 0;                           // nothing to count: nothing is launched
    REQUIRE(hist && (uintptr_t)hist % 4 == 0, "sf_sslcolor_hist_u8: hist must be a 4-byte aligned pointer");
    p.hist = hist;
    p.vec = u8_frames_vec(src, nullptr, p.slab);
    hipLaunchKernelGGL(sf_sslcolor_hist_zero_kernel, dim3(N), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    if (check_launch("sslcolor_hist_zero")) return -1;
    hipLaunchKernelGGL(sf_sslcolor_hist_kernel, dim3(cdiv(p.slab, SF_U8_CHUNK), N * T), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("sslcolor_hist");
}
extern "C" int sf_sslcolor_stream_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws,
                                     const int32_t* table_host, const int32_t* table_dev, const int32_t* hist, sf_stream_t stream) {
    SslColorParams p;
    if (fill_u8_frames("sf_sslcolor_stream_u8", p, src, N, T, Hs, Ws, table_dev)) return -1;
    const int64_t bytes = (int64_t)N * T * p.slab * 3;
    REQUIRE(dst, "sf_sslcolor_stream_u8: null dst");
    REQUIRE(dst == src || (const unsigned char*)dst + bytes <= (const unsigned char*)src || (const unsigned char*)src + bytes <= (const unsigned char*)dst,
            "sf_sslcolor_stream_u8: dst must be src itself (in place) or must not overlap it");
    int hist_rows, stream_rows, blur_rows;
    if (check_sslcolor_table("sf_sslcolor_stream_u8", table_host, N, Hs, Ws, hist_rows, stream_rows, blur_rows)) return -1;
    REQUIRE(hist_rows == 0 || hist, "sf_sslcolor_stream_u8: a row with contrast needs the histograms");
    if (stream_rows == 0 && dst == src) return 0;           // in place and nothing drawn: nothing is launched
    p.dst = (unsigned char*)dst; p.hist = const_cast<int32_t*>(hist);
    p.vec = u8_frames_vec(src, dst, p.slab);
    hipLaunchKernelGGL(sf_sslcolor_stream_kernel, dim3(cdiv(p.slab, SF_U8_CHUNK), N * T), dim3(SF_THREADS), 0,
                       (hipStream_t)stream, p);
    return check_launch("sslcolor_stream");
}
static int sslcolor_blur(const char* who, bool cols, const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws,
                         const int32_t* table_host, const int32_t* table_dev, sf_stream_t stream) {
    SslColorParams p;
    if (fill_u8_frames(who, p, src, N, T, Hs, Ws, table_dev)) return -1;
    const int64_t bytes = (int64_t)N * T * p.slab * 3;
    REQUIRE(dst && ((const unsigned char*)dst + bytes <= (const unsigned char*)src || (const unsigned char*)src + bytes <= (const unsigned char*)dst),
            "%s: dst must be another buffer than src", who);
    REQUIRE(Ws <= SF_SSLCOLOR_MAX_W, "%s: frames wider than %d pixels are not supported", who, SF_SSLCOLOR_MAX_W);
    REQUIRE(N <= 65535 && (int64_t)T * Hs < (1 << 24), "%s: bad shape (N <= 65535, T * Hs < 2^24)", who);
    int hist_rows, stream_rows, blur_rows;
    if (check_sslcolor_table(who, table_host, N, Hs, Ws, hist_rows, stream_rows, blur_rows)) return -1;
    if (blur_rows == 0) return 0;                           // nothing is launched
    p.dst = (unsigned char*)dst;
    const int stack = T * Hs;
    if (cols) {
        p.vec = Ws % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0;
        hipLaunchKernelGGL(sf_sslcolor_blur_cols_kernel, dim3(cdiv(Ws, SF_SSLCOLOR_COLS), cdiv(stack, SF_SSLCOLOR_RUN), N),
                           dim3(SF_THREADS), 0, (hipStream_t)stream, p);
        return check_launch("sslcolor_blur_cols");
    }
    p.rows = SF_SSLCOLOR_ROW_LDS / (3 * Ws);                // >= 1: Ws <= SF_SSLCOLOR_MAX_W
    if (p.rows > 8) p.rows = 8;
    hipLaunchKernelGGL(sf_sslcolor_blur_rows_kernel, dim3(cdiv(stack, p.rows), N), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("sslcolor_blur_rows");
}
extern "C" int sf_sslcolor_blur_rows_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws,
                                        const int32_t* table_host, const int32_t* table_dev, sf_stream_t stream) {
    return sslcolor_blur("sf_sslcolor_blur_rows_u8", false, src, dst, N, T, Hs, Ws, table_host, table_dev, stream);
}
extern "C" int sf_sslcolor_blur_cols_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws,
                                        const int32_t* table_host, const int32_t* table_dev, sf_stream_t stream) {
    return sslcolor_blur("sf_sslcolor_blur_cols_u8", true, src, dst, N, T, Hs, Ws, table_host, table_dev, stream);
}

static int row_scale_add_impl(const void* x, int32_t ldx, const float* scale, int64_t rows_per_sample, const void* resid,
                              int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C, const sf_rows32* side,
                              sf_stream_t stream) {
    REQUIRE(x && scale && y, "sf_row_scale_add: null pointer");
    if (check_rows("sf_row_scale_add", M, C)) return -1;
    REQUIRE(rows_per_sample > 0 && rows_per_sample < (1ll << 31), "sf_row_scale_add: bad rows_per_sample");
    REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && (!resid || ldr % 8 == 0), "sf_row_scale_add: pitches must be multiples of 8");
    RowScaleParams p;
    p.x = (const f16*)x; p.ldx = ldx; p.scale = scale; p.resid = (const f16*)resid; p.ldr = ldr;
    p.y = (f16*)y; p.ldy = ldy;
    if (rows32_arg("sf_row_scale_add_rows32", side, M, C, true, p.f32)) return -1;
    p.total = M * (C / 8);
    REQUIRE(p.total < (1ll << 31), "sf_row_scale_add: too many elements");
    p.fdG = make_fastdiv(C / 8); p.fdRows = make_fastdiv((uint32_t)rows_per_sample);
    hipLaunchKernelGGL(sf_row_scale_add_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("row_scale_add");
}
extern "C" int sf_row_scale_add(const void* x, int32_t ldx, const float* scale, int64_t rows_per_sample, const void* resid,
                                int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C, sf_stream_t stream) {
    return row_scale_add_impl(x, ldx, scale, rows_per_sample, resid, ldr, y, ldy, M, C, nullptr, stream);
}
extern "C" int sf_row_scale_add_rows32(const void* x, int32_t ldx, const float* scale, int64_t rows_per_sample,
                                       const void* resid, int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C,
                                       const sf_rows32* side, sf_stream_t stream) {
    REQUIRE(side, "sf_row_scale_add_rows32: null side rows");
    return row_scale_add_impl(x, ldx, scale, rows_per_sample, resid, ldr, y, ldy, M, C, side, stream);
}

extern "C" int sf_transpose_heads(const void* x, int32_t ldx, void* xt, int32_t ldk, int32_t B, int32_t Nk, int32_t heads,
                                  int32_t D, sf_stream_t stream) {
    REQUIRE(x && xt && ldk % 8 == 0 && ldk >= Nk && B > 0 && heads > 0 && D > 0, "sf_transpose_heads: bad arguments");
    TransposeParams p;
    p.x = (const f16*)x; p.ldx = ldx; p.xt = (f16*)xt; p.ldk = ldk; p.B = B; p.Nk = Nk; p.heads = heads; p.D = D;
    p.total = (int64_t)B * heads * D * (ldk / 8);
    REQUIRE(p.total < (1ll << 31), "sf_transpose_heads: too many elements");
    p.fdK8 = make_fastdiv(ldk / 8); p.fdD = make_fastdiv(D); p.fdHeads = make_fastdiv(heads);
    hipLaunchKernelGGL(sf_transpose_heads_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("transpose_heads");
}

// ================================================================================================
// X3D: per-sample channel means, SE gate, gate * BatchNorm -> Swish/ReLU
static const int kSampleChunks = 64;
static int sample_plan(int64_t S, int C, RowTile& rt, dim3& grid) {
    rt = make_rowtile(S, C, kSampleChunks, grid);
    return (int)grid.x;
}
extern "C" int sf_sample_chunks(int64_t S, int32_t C) {
    if (check_rows("sf_sample_chunks", S, C)) return -1;
    RowTile rt;
    dim3 grid;
    return sample_plan(S, C, rt, grid);
}
static int sample_sum(int mode, int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                      const float* shift, int relu, const void* dz, int32_t lddz, const float* gate, int swish,
                      float* part, float* out, float inv_count, hipStream_t s) {
    if (check_rows("sf_sample_sum", S, C)) return -1;
    REQUIRE(N > 0 && N <= 65535 && y && part && out, "sf_sample_sum: bad arguments");
    REQUIRE((scale == nullptr) == (shift == nullptr), "sf_sample_sum: scale/shift must come together");
    SampleSumParams p;
    memset(&p, 0, sizeof(p));
    dim3 grid;
    const int chunks = sample_plan(S, C, p.rt, grid);
    REQUIRE(grid.y == 1, "sf_sample_sum: C > 2048 is not supported");
    grid.z = N;
    p.S = S; p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.relu = relu; p.mode = mode;
    p.dz = (const f16*)dz; p.lddz = lddz; p.gate = gate; p.swish = swish; p.part = part;
    hipLaunchKernelGGL(sf_sample_sum_kernel, grid, dim3(SF_THREADS), 0, s, p);
    if (check_launch("sample_sum")) return -1;
    hipLaunchKernelGGL(sf_sample_fold_kernel, dim3(cdiv(C, SF_THREADS), N), dim3(SF_THREADS), 0, s, (const float*)part, chunks,
                       C, inv_count, out);
    return check_launch("sample_fold");
}
extern "C" int sf_sample_mean(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                              const float* shift, int relu, float* part, float* out, sf_stream_t stream) {
    return sample_sum(0, N, S, C, y, ldy, scale, shift, relu, nullptr, 0, nullptr, 0, part, out, 1.0f / (float)S,
                      (hipStream_t)stream);
}
extern "C" int sf_gate_grad(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                            const float* shift, const void* dz, int32_t lddz, const float* gate, int swish, float* part,
                            float* dgate, sf_stream_t stream) {
    REQUIRE(dz && scale, "sf_gate_grad: null pointer");
    return sample_sum(1, N, S, C, y, ldy, scale, shift, 0, dz, lddz, gate, swish, part, dgate, 1.0f, (hipStream_t)stream);
}
// One pass over y and dz for the backward of SE-gated Swish (X3DTransform, resnet_helper.py:226-250): du0 = dz * act'(gate * u) * gate
// is stored, sums[n][0] = the gate's gradient sum_pos dz * act'(gate * u) * u, sums[n][1] = sum_pos du0, sums[n][2] = sum_pos du0 * y
// (stored 16-bit du0: what sf_bn_bwd_reduce would sum).  part: [N * sf_sample_chunks(S, C)][4][C] scratch.
extern "C" int sf_gate_bwd_sums(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                                const float* shift, const void* dz, int32_t lddz, const float* gate, int swish, void* du0,
                                int32_t lddu, float* part, float* sums, sf_stream_t stream) {
    if (check_rows("sf_gate_bwd_sums", S, C)) return -1;
    REQUIRE(N > 0 && N <= 65535 && y && dz && scale && shift && du0 && part && sums, "sf_gate_bwd_sums: bad arguments");
    SampleSumParams p;
    memset(&p, 0, sizeof(p));
    dim3 grid;
    const int chunks = sample_plan(S, C, p.rt, grid);
    REQUIRE(grid.y == 1, "sf_gate_bwd_sums: C > 2048 is not supported");
    grid.z = N;
    p.S = S; p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.mode = 2;
    p.dz = (const f16*)dz; p.lddz = lddz; p.gate = gate; p.swish = swish; p.part = part; p.z = (f16*)du0; p.ldz = lddu;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sf_sample_sum_kernel, grid, dim3(SF_THREADS), 0, s, p);
    if (check_launch("gate_bwd_sums")) return -1;
    hipLaunchKernelGGL(sf_sample_fold3_kernel, dim3(cdiv(C, SF_THREADS), N, 3), dim3(SF_THREADS), 0, s, (const float*)part, chunks, C, sums);
    return check_launch("gate_bwd_sums_fold");
}
static int fill_se(SeGateParams& p, int32_t C, int32_t Cp, int32_t F, const float* w1, const float* b1, const float* w2,
                   const float* b2) {
    REQUIRE(C > 0 && C <= Cp && Cp <= 1024 && F > 0 && F <= 1024, "SE gate: C, F must be <= 1024");
    REQUIRE(w1 && b1 && w2 && b2, "SE gate: null weights");
    memset(&p, 0, sizeof(p));
    p.C = C; p.Cp = Cp; p.F = F; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2;
    return 0;
}
extern "C" int sf_se_gate_fwd(int32_t N, int32_t C, int32_t Cp, int32_t F, const float* m, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* h, float* gate, sf_stream_t stream) {
    SeGateParams p;
    if (fill_se(p, C, Cp, F, w1, b1, w2, b2)) return -1;
    REQUIRE(m && h && gate && N > 0, "sf_se_gate_fwd: null pointer");
    p.m = m; p.h = h; p.gate = gate;
    hipLaunchKernelGGL(sf_se_gate_fwd_kernel, dim3(N), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("se_gate_fwd");
}
extern "C" int sf_se_gate_bwd(int32_t N, int32_t C, int32_t Cp, int32_t F, const float* gate, const float* h,
                              const float* w1, const float* w2, const float* dgate, float* dpre2, float* dpre1, float* dm,
                              sf_stream_t stream) {
    SeGateParams p;
    if (fill_se(p, C, Cp, F, w1, w1, w2, w2)) return -1;
    REQUIRE(gate && h && dgate && dpre2 && dpre1 && dm && N > 0, "sf_se_gate_bwd: null pointer");
    p.gate = (float*)gate; p.h = (float*)h; p.dgate = dgate; p.dpre2 = dpre2; p.dpre1 = dpre1; p.dm = dm;
    hipLaunchKernelGGL(sf_se_gate_bwd_kernel, dim3(N), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("se_gate_bwd");
}
extern "C" int sf_outer_sum(const float* a, int32_t lda, const float* b, int32_t ldb, int32_t N, int32_t I, int32_t J,
                            float* out, float scale, int accumulate, sf_stream_t stream) {
    REQUIRE(a && out && N > 0 && I > 0 && J > 0 && (b || J == 1), "sf_outer_sum: bad arguments");
    hipLaunchKernelGGL(sf_outer_sum_kernel, dim3(cdiv((int64_t)I * J, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream,
                       a, lda, b, ldb, N, I, J, out, scale, accumulate);
    return check_launch("outer_sum");
}
static int fill_gate_act(GateActParams& p, int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                         const float* shift, const float* gate, int swish, dim3& grid, int max_blocks = 8192) {
    if (check_rows("gate_act", (int64_t)N * S, C)) return -1;
    REQUIRE(y && scale && shift, "gate_act: null pointer");
    memset(&p, 0, sizeof(p));
    p.rt = make_rowtile((int64_t)N * S, C, max_blocks, grid);
    p.S = S; p.y = (const f16*)y; p.ldy = ldy; p.scale = scale; p.shift = shift; p.gate = gate; p.swish = swish;
    p.fdS = make_fastdiv((uint32_t)S);
    return 0;
}
extern "C" int sf_gate_act_fwd(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                               const float* shift, const float* gate, int swish, void* z, int32_t ldz, sf_stream_t stream) {
    GateActParams p;
    dim3 grid;
    if (fill_gate_act(p, N, S, C, y, ldy, scale, shift, gate, swish, grid)) return -1;
    REQUIRE(z != nullptr, "sf_gate_act_fwd: null pointer");
    p.z = (f16*)z; p.ldz = ldz;
    hipLaunchKernelGGL(sf_gate_act_fwd_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("gate_act_fwd");
}
extern "C" int sf_gate_act_bwd(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                               const float* shift, const float* gate, int swish, const void* dz, int32_t lddz,
                               const float* dmean, void* du, int32_t lddu, sf_stream_t stream) {
    GateActParams p;
    dim3 grid;
    if (fill_gate_act(p, N, S, C, y, ldy, scale, shift, gate, swish, grid)) return -1;
    REQUIRE(dz && du, "sf_gate_act_bwd: null pointer");
    p.dz = (const f16*)dz; p.lddz = lddz; p.dmean = dmean; p.inv_S = 1.0f / (float)S; p.z = (f16*)du; p.ldz = lddu;
    hipLaunchKernelGGL(sf_gate_act_bwd_kernel<false>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("gate_act_bwd");
}
// ... with the reduction of the BatchNorm backward that follows fused in: bn_part[sf_gate_act_bwd_bn_rows()][2][C] gets the column
// sums of du and du * y (X3DTransform: the BatchNorm between the channelwise 3x3x3 convolution and SE / Swish,
// resnet_helper.py:226-250); 2048 workgroups at most, so that sf_bn_bwd_finalize needs no fold stage
static const int kGateBnBlocks = 2048;
extern "C" int sf_gate_act_bwd_bn_rows(int32_t N, int64_t S, int32_t C) {
    if (check_rows("gate_act", (int64_t)N * S, C)) return -1;
    dim3 grid;
    make_rowtile((int64_t)N * S, C, kGateBnBlocks, grid);
    return (int)grid.x;
}
extern "C" int sf_gate_act_bwd_bn(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale,
                                  const float* shift, const float* gate, int swish, const void* dz, int32_t lddz,
                                  const float* dmean, void* du, int32_t lddu, float* bn_part, sf_stream_t stream) {
    GateActParams p;
    dim3 grid;
    if (fill_gate_act(p, N, S, C, y, ldy, scale, shift, gate, swish, grid, kGateBnBlocks)) return -1;
    REQUIRE(dz && du && bn_part, "sf_gate_act_bwd_bn: null pointer");
    p.dz = (const f16*)dz; p.lddz = lddz; p.dmean = dmean; p.inv_S = 1.0f / (float)S; p.z = (f16*)du; p.ldz = lddu;
    p.bn_part = bn_part;
    hipLaunchKernelGGL(sf_gate_act_bwd_kernel<true>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("gate_act_bwd_bn");
}


// ================================================================================================
// Training-step glue on the flat gradient memory (sf_optim.h; replaces tools/train_net.py:150-172 + optimizer.step()).
static const int kFlatBlocks = 1024;
extern "C" int sf_flat_blocks(int64_t n) {
    if (n <= 0) return fail("sf_flat_blocks: empty buffer");
    int64_t b = (n / 4 + SF_THREADS - 1) / SF_THREADS;
    return (int)(b < 1 ? 1 : (b > kFlatBlocks ? kFlatBlocks : b));
}
extern "C" int sf_flat_sumsq(const float* g, int64_t n, float* part, sf_stream_t stream) {
    REQUIRE(g && part && n > 0, "sf_flat_sumsq: bad arguments");
    REQUIRE((uintptr_t)g % 4 == 0, "sf_flat_sumsq: the buffer must be 4-byte aligned");
    FlatSumsqParams p;
    p.g = g; p.n = n; p.part = part;
    hipLaunchKernelGGL(sf_flat_sumsq_kernel, dim3(sf_flat_blocks(n)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_sumsq");
}
extern "C" int sf_step_control(const float* part, int32_t nblk, float* ctl, float world, float clip_norm, int dynamic,
                               float growth, float backoff, int32_t growth_interval, sf_stream_t stream) {
    REQUIRE(part && ctl && nblk > 0 && world >= 1.f, "sf_step_control: bad arguments");
    REQUIRE(!dynamic || (growth >= 1.f && backoff > 0.f && backoff <= 1.f && growth_interval >= 1), "sf_step_control: bad GradScaler constants");
    StepControlParams p;
    p.part = part; p.nblk = nblk; p.ctl = ctl; p.world = world; p.clip_norm = clip_norm; p.dynamic = dynamic;
    p.growth = growth; p.backoff = backoff; p.growth_interval = growth_interval;
    hipLaunchKernelGGL(sf_step_control_kernel, dim3(1), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("step_control");
}
static int fill_flat_update(FlatUpdateParams& p, float* param, const float* grad, float* m1, float* m2, const void* segs,
                            const int32_t* blk_seg, const int32_t* blk_off, const float* ctl, const float* lr, const float* wd,
                            int32_t ngroups, float clip_val) {
    REQUIRE(param && grad && segs && blk_seg && blk_off && ctl && lr && wd, "flat update: null pointer");
    REQUIRE(ngroups >= 1 && ngroups <= SF_OPT_MAX_GROUPS, "flat update: 1..%d parameter groups", SF_OPT_MAX_GROUPS);
    memset(&p, 0, sizeof(p));
    p.param = param; p.grad = grad; p.m1 = m1; p.m2 = m2; p.segs = (const FlatSeg*)segs; p.blk_seg = blk_seg; p.blk_off = blk_off;
    p.ctl = ctl; p.clip_val = clip_val;
    for (int g = 0; g < ngroups; ++g) { p.lr[g] = lr[g]; p.wd[g] = wd[g]; }   // host arrays (a handful of floats per step)
    return 0;
}
extern "C" int sf_flat_sgd(float* param, const float* grad, float* mom, const void* segs, const int32_t* blk_seg,
                           const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* lr, const float* wd,
                           int32_t ngroups, float clip_val, float momentum, float dampening, int nesterov, sf_stream_t stream) {
    FlatUpdateParams p;
    if (fill_flat_update(p, param, grad, mom, nullptr, segs, blk_seg, blk_off, ctl, lr, wd, ngroups, clip_val)) return -1;
    REQUIRE(nblocks > 0 && (momentum == 0.f || mom), "sf_flat_sgd: momentum needs a buffer");
    p.momentum = momentum; p.dampening = dampening; p.nesterov = nesterov;
    hipLaunchKernelGGL(sf_flat_sgd_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_sgd");
}
extern "C" int sf_flat_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const void* segs,
                             const int32_t* blk_seg, const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* lr,
                             const float* wd, int32_t ngroups, float clip_val, float beta1, float beta2, float eps,
                             sf_stream_t stream) {
    FlatUpdateParams p;
    if (fill_flat_update(p, param, grad, exp_avg, exp_avg_sq, segs, blk_seg, blk_off, ctl, lr, wd, ngroups, clip_val)) return -1;
    REQUIRE(nblocks > 0 && exp_avg && exp_avg_sq, "sf_flat_adamw: moment buffers");
    p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    hipLaunchKernelGGL(sf_flat_adamw_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_adamw");
}

// Table-driven update (ABI 24): per-group hyper-parameters in device memory, any number of groups, optional LARS
// (slowfast/models/optimizer.py:146-237 and :262-359).
static int fill_flat_tab(FlatTabParams& p, float* param, const float* grad, float* m1, float* m2, const void* segs,
                         const int32_t* blk_seg, const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* hyper,
                         const float* trust, float clip_val) {
    REQUIRE(param && grad && segs && blk_seg && blk_off && ctl && hyper && nblocks > 0, "flat table update: bad arguments");
    REQUIRE((uintptr_t)hyper % 16 == 0, "flat table update: hyper must be 16-byte aligned");
    memset(&p, 0, sizeof(p));
    p.param = param; p.grad = grad; p.m1 = m1; p.m2 = m2; p.segs = (const FlatSeg*)segs; p.blk_seg = blk_seg; p.blk_off = blk_off;
    p.ctl = ctl; p.hyper = hyper; p.trust = trust; p.clip_val = clip_val;
    return 0;
}
extern "C" int sf_flat_sgd_tab(float* param, const float* grad, float* mom, const void* segs, const int32_t* blk_seg,
                               const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* hyper, const float* trust,
                               float clip_val, float momentum, float dampening, int nesterov, sf_stream_t stream) {
    FlatTabParams p;
    if (fill_flat_tab(p, param, grad, mom, nullptr, segs, blk_seg, blk_off, nblocks, ctl, hyper, trust, clip_val)) return -1;
    REQUIRE(momentum == 0.f || mom, "sf_flat_sgd_tab: momentum needs a buffer");
    p.momentum = momentum; p.dampening = dampening; p.nesterov = nesterov;
    hipLaunchKernelGGL(sf_flat_sgd_tab_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_sgd_tab");
}
extern "C" int sf_flat_adamw_tab(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const void* segs,
                                 const int32_t* blk_seg, const int32_t* blk_off, int32_t nblocks, const float* ctl,
                                 const float* hyper, const float* trust, float clip_val, float beta1, float beta2, float eps,
                                 sf_stream_t stream) {
    FlatTabParams p;
    if (fill_flat_tab(p, param, grad, exp_avg, exp_avg_sq, segs, blk_seg, blk_off, nblocks, ctl, hyper, trust, clip_val)) return -1;
    REQUIRE(exp_avg && exp_avg_sq, "sf_flat_adamw_tab: moment buffers");
    p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    hipLaunchKernelGGL(sf_flat_adamw_tab_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_adamw_tab");
}
extern "C" int sf_flat_lars_trust(const float* param, const float* grad, const void* segs, const int32_t* blk_seg,
                                  const int32_t* blk_off, int32_t nblocks, const int32_t* seg_row, int32_t nseg, const float* ctl,
                                  const float* hyper, double* part, float* trust, float clip_val, float trust_coef, float eps,
                                  sf_stream_t stream) {
    REQUIRE(param && grad && segs && blk_seg && blk_off && seg_row && ctl && hyper && part && trust, "sf_flat_lars_trust: null pointer");
    REQUIRE(nblocks > 0 && nseg > 0 && nseg <= nblocks && trust_coef > 0.f && eps >= 0.f, "sf_flat_lars_trust: bad arguments");
    FlatLarsParams p;
    p.param = param; p.grad = grad; p.segs = (const FlatSeg*)segs; p.blk_seg = blk_seg; p.blk_off = blk_off; p.seg_row = seg_row;
    p.ctl = ctl; p.hyper = hyper; p.part = part; p.trust = trust; p.clip_val = clip_val; p.trust_coef = trust_coef; p.eps = eps;
    hipLaunchKernelGGL(sf_flat_lars_norms_kernel, dim3(nblocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    if (check_launch("flat_lars_norms")) return -1;
    hipLaunchKernelGGL(sf_flat_lars_trust_kernel, dim3(nseg), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("flat_lars_trust");
}

// ================================================================================================
// MaskFeat step glue (sf_hog.h, sf_tokens.h): HOG regression targets of the clip in one launch, mask-token substitution after
// the patch embedding and its backward.  Kernel launches only.
extern "C" int sf_hog_targets_f32(const float* clip, int32_t B, int32_t T, int32_t H, int32_t W, int32_t ts, int32_t fs,
                                  float* out, sf_stream_t stream) {
    REQUIRE(clip && out, "sf_hog_targets_f32: null pointer");
    REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && ts > 0 && fs > 0, "sf_hog_targets_f32: bad shape");
    REQUIRE(H == W, "sf_hog_targets_f32: H != W (%d x %d): the targets are defined for square clips", H, W);
    REQUIRE(H % (SF_HOG_CELL * fs) == 0, "sf_hog_targets_f32: H %% (8 * fs) != 0 (H=%d, fs=%d): u = (H / 8) / fs must be a "
            "whole number >= 1", H, fs);
    HogParams p;
    p.x = clip; p.out = out; p.T = T; p.H = H; p.W = W; p.ts = ts; p.Tu = (T + ts - 1) / ts; p.fs = fs;
    p.u = H / SF_HOG_CELL / fs;
    REQUIRE(p.u >= 1, "sf_hog_targets_f32: u < 1");
    p.F = 3 * SF_HOG_BINS * p.u * p.u;
    REQUIRE(SF_HOG_CELL * p.u <= SF_HOG_TILE_W && p.F <= SF_HOG_STAGE,
            "sf_hog_targets_f32: u = %d cells per token side is beyond the built tile (u <= 17)", p.u);
    int nj = SF_HOG_TILE_W / (SF_HOG_CELL * p.u);
    if (nj > SF_HOG_STAGE / p.F) nj = SF_HOG_STAGE / p.F;
    if (nj > fs) nj = fs;
    p.nj = nj;
    const int64_t gz = (int64_t)B * p.Tu;
    REQUIRE(gz <= 65535 && fs <= 65535, "sf_hog_targets_f32: more than 65535 (sample, frame) pairs");
    REQUIRE((int64_t)B * 3 * T * H * W < (1ll << 40), "sf_hog_targets_f32: clip too large");
    const dim3 grid(cdiv(fs, nj), fs, (unsigned)gz);
    if (nj * p.F <= SF_HOG_STAGE_SMALL)
        hipLaunchKernelGGL(sf_hog_targets_kernel<SF_HOG_STAGE_SMALL>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(sf_hog_targets_kernel<SF_HOG_STAGE>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("hog_targets_f32");
}

static int fill_masktok(const char* who, MaskTokParams& p, int32_t B, int32_t cls, int32_t T, int32_t H, int32_t W, int32_t C,
                        const void* mask, int32_t Tw, int32_t Hw, int32_t Ww) {
    REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= 2048 && (cls == 0 || cls == 1), "%s: bad shape", who);
    REQUIRE(mask && Tw > 0 && Hw > 0 && Ww > 0, "%s: null mask table", who);
    REQUIRE(Tw == T, "%s: the mask table has Tw = %d windows in time, the token grid T' = %d (Tw != T')", who, Tw, T);
    REQUIRE(H % Hw == 0 && W % Ww == 0, "%s: the mask window grid %d x %d does not divide the token grid %d x %d", who, Hw, Ww,
            H, W);
    memset(&p, 0, sizeof(p));
    p.mask = (const uint8_t*)mask; p.B = B; p.cls = cls; p.N = T * H * W; p.C = C;
    p.H = H; p.W = W; p.Hw = Hw; p.Ww = Ww; p.rh = H / Hw; p.rw = W / Ww;
    REQUIRE((int64_t)B * (p.N + cls) * (C / 8) < (1ll << 31), "%s: too many elements", who);
    p.fdG = make_fastdiv((uint32_t)(C / 8)); p.fdN = make_fastdiv((uint32_t)p.N);
    p.fdW = make_fastdiv((uint32_t)W); p.fdH = make_fastdiv((uint32_t)H);
    p.groups = SF_THREADS / (C / 8);
    return 0;
}
extern "C" int sf_mask_tokens_fwd(void* x, int32_t ldx, int32_t B, int32_t cls, int32_t T, int32_t H, int32_t W, int32_t C,
                                  const void* mask, int32_t Tw, int32_t Hw, int32_t Ww, const float* mask_token,
                                  const float* pos, sf_stream_t stream) {
    MaskTokParams p;
    if (fill_masktok("sf_mask_tokens_fwd", p, B, cls, T, H, W, C, mask, Tw, Hw, Ww)) return -1;
    REQUIRE(x && mask_token && ldx >= C && ldx % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)mask_token % 16 == 0 &&
            (uintptr_t)pos % 16 == 0, "sf_mask_tokens_fwd: bad pointer / pitch");
    p.x = (f16*)x; p.ldx = ldx; p.tok = mask_token; p.pos = pos;
    p.total = (int64_t)B * p.N * (C / 8);
    hipLaunchKernelGGL(sf_mask_tokens_fwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("mask_tokens_fwd");
}
extern "C" int sf_mask_tokens_bwd_blocks(int32_t rows, int32_t C) {
    REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 2048, "sf_mask_tokens_bwd_blocks: bad shape");
    const int groups = SF_THREADS / (C / 8);
    return cdiv(rows, groups * SF_MASKTOK_RPT) * groups;
}
extern "C" int sf_mask_tokens_bwd(const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t B, int32_t cls, int32_t T,
                                  int32_t H, int32_t W, int32_t C, const void* mask, int32_t Tw, int32_t Hw, int32_t Ww,
                                  float* dpos, float* part, sf_stream_t stream) {
    MaskTokParams p;
    if (fill_masktok("sf_mask_tokens_bwd", p, B, cls, T, H, W, C, mask, Tw, Hw, Ww)) return -1;
    REQUIRE(dy && dx && part && lddy >= C && lddy % 8 == 0 && lddx >= C && lddx % 8 == 0 && (uintptr_t)dy % 16 == 0 &&
            (uintptr_t)dx % 16 == 0 && (uintptr_t)dpos % 16 == 0 && (uintptr_t)part % 16 == 0,
            "sf_mask_tokens_bwd: bad pointer / pitch");
    p.dy = (const f16*)dy; p.lddy = lddy; p.x = (f16*)dx; p.ldx = lddx; p.dpos = dpos; p.part = part;
    const int blocks = cdiv(p.N + cls, p.groups * SF_MASKTOK_RPT);
    hipLaunchKernelGGL(sf_mask_tokens_bwd_kernel, dim3(blocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("mask_tokens_bwd");
}

// ================================================================================================
// MAE step glue (sf_tokens.h, sf_pixel.h): the encoder's kept-token gather, the decoder's token assembly, their backwards and
// the pixel regression targets.  Kernel launches only.
static int fill_tokids(const char* who, TokIdsParams& p, int32_t B, int32_t cls, int32_t L, int32_t K, int32_t C,
                       const int32_t* ids) {
    REQUIRE(B > 0 && L > 0 && C > 0 && C % 8 == 0 && C <= 2048 && (cls == 0 || cls == 1), "%s: bad shape", who);
    REQUIRE(K > 0 && K <= L, "%s: K = %d kept tokens of L = %d (0 < K <= L)", who, K, L);
    REQUIRE(ids && (uintptr_t)ids % 4 == 0, "%s: null ids_restore table", who);
    memset(&p, 0, sizeof(p));
    p.ids = ids; p.B = B; p.cls = cls; p.L = L; p.K = K; p.C = C;
    p.total = (int64_t)B * (cls + L) * (C / 8);
    REQUIRE(p.total < (1ll << 31), "%s: too many elements", who);
    p.fdG = make_fastdiv((uint32_t)(C / 8)); p.fdN = make_fastdiv((uint32_t)(cls + L));
    p.groups = SF_THREADS / (C / 8);
    return 0;
}
static bool tok_rows_ok(const void* ptr, int32_t ld, int32_t C) { return ptr && ld >= C && ld % 8 == 0 && (uintptr_t)ptr % 16 == 0; }

extern "C" int sf_token_keep_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t B, int32_t cls, int32_t L, int32_t K,
                                 int32_t C, const int32_t* ids, sf_stream_t stream) {
    TokIdsParams p;
    if (fill_tokids("sf_token_keep_fwd", p, B, cls, L, K, C, ids)) return -1;
    REQUIRE(tok_rows_ok(x, ldx, C) && tok_rows_ok(y, ldy, C), "sf_token_keep_fwd: bad pointer / pitch");
    p.x = (const f16*)x; p.ldx = ldx; p.y = (f16*)y; p.ldy = ldy;
    hipLaunchKernelGGL(sf_token_keep_fwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("token_keep_fwd");
}
extern "C" int sf_token_keep_bwd(const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t B, int32_t cls, int32_t L,
                                 int32_t K, int32_t C, const int32_t* ids, sf_stream_t stream) {
    TokIdsParams p;
    if (fill_tokids("sf_token_keep_bwd", p, B, cls, L, K, C, ids)) return -1;
    REQUIRE(tok_rows_ok(dy, lddy, C) && tok_rows_ok(dx, lddx, C), "sf_token_keep_bwd: bad pointer / pitch");
    p.x = (const f16*)dy; p.ldx = lddy; p.y = (f16*)dx; p.ldy = lddx;
    hipLaunchKernelGGL(sf_token_keep_bwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("token_keep_bwd");
}
extern "C" int sf_token_restore_fwd(const void* e, int32_t lde, void* y, int32_t ldy, int32_t B, int32_t cls, int32_t L,
                                    int32_t K, int32_t C, const int32_t* ids, const float* mask_token, const float* dpos,
                                    sf_stream_t stream) {
    TokIdsParams p;
    if (fill_tokids("sf_token_restore_fwd", p, B, cls, L, K, C, ids)) return -1;
    REQUIRE(tok_rows_ok(e, lde, C) && tok_rows_ok(y, ldy, C) && mask_token && dpos && (uintptr_t)mask_token % 16 == 0 &&
            (uintptr_t)dpos % 16 == 0, "sf_token_restore_fwd: bad pointer / pitch");
    p.x = (const f16*)e; p.ldx = lde; p.y = (f16*)y; p.ldy = ldy; p.tok = mask_token; p.pos = dpos;
    hipLaunchKernelGGL(sf_token_restore_fwd_kernel, dim3(pool_grid(p.total)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("token_restore_fwd");
}
extern "C" int sf_token_restore_bwd_blocks(int32_t rows, int32_t C) {
    REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 2048, "sf_token_restore_bwd_blocks: bad shape");
    const int groups = SF_THREADS / (C / 8);
    return cdiv(rows, groups * SF_TOKRESTORE_RPT) * groups;
}
extern "C" int sf_token_restore_bwd(const void* dy, int32_t lddy, void* de, int32_t ldde, int32_t B, int32_t cls, int32_t L,
                                    int32_t K, int32_t C, const int32_t* ids, float* d_dpos, float* part, sf_stream_t stream) {
    TokIdsParams p;
    if (fill_tokids("sf_token_restore_bwd", p, B, cls, L, K, C, ids)) return -1;
    REQUIRE(tok_rows_ok(dy, lddy, C) && tok_rows_ok(de, ldde, C) && part && (uintptr_t)part % 16 == 0 &&
            (uintptr_t)d_dpos % 16 == 0, "sf_token_restore_bwd: bad pointer / pitch");
    p.x = (const f16*)dy; p.ldx = lddy; p.y = (f16*)de; p.ldy = ldde; p.dpos = d_dpos; p.part = part;
    const int blocks = cdiv(cls + L, p.groups * SF_TOKRESTORE_RPT);
    hipLaunchKernelGGL(sf_token_restore_bwd_kernel, dim3(blocks), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("token_restore_bwd");
}

extern "C" int sf_pixel_targets_f32(const float* clip, int32_t B, int32_t T, int32_t H, int32_t W, int32_t ts, int32_t u,
                                    int32_t p_, int32_t norm, float* out, sf_stream_t stream) {
    REQUIRE(clip && out, "sf_pixel_targets_f32: null pointer");
    REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && ts > 0 && u > 0 && p_ > 0, "sf_pixel_targets_f32: bad shape");
    REQUIRE(H == W, "sf_pixel_targets_f32: H != W (%d x %d): the targets are defined for square clips", H, W);
    REQUIRE(H % p_ == 0, "sf_pixel_targets_f32: H %% p != 0 (H=%d, p=%d)", H, p_);
    REQUIRE(T % ts == 0, "sf_pixel_targets_f32: T %% ts != 0 (T=%d, ts=%d)", T, ts);
    REQUIRE(u == 1 || u == ts, "sf_pixel_targets_f32: u = %d frames per token: u must be 1 (TIME_STRIDE_LOSS) or ts = %d", u, ts);
    const int64_t n = (int64_t)u * p_ * p_ * 3;
    REQUIRE(n <= SF_PIXEL_STAGE, "sf_pixel_targets_f32: a row of u * p * p * 3 = %lld values is beyond the staged row (<= %d)",
            (long long)n, SF_PIXEL_STAGE);
    PixelParams p;
    p.x = clip; p.out = out; p.T = T; p.H = H; p.W = W; p.ts = ts; p.Tt = T / ts; p.u = u; p.p = p_;
    p.h = H / p_; p.w = W / p_; p.n = (int)n; p.norm = norm ? 1 : 0;
    const int njmax = SF_PIXEL_STAGE / p.n < p.w ? SF_PIXEL_STAGE / p.n : p.w;
    const int chunks = cdiv(p.w, njmax);
    p.nj = cdiv(p.w, chunks);                              // balanced chunks: 14 tokens of 768 values -> 7 + 7
    p.fdRun = make_fastdiv((uint32_t)(p.nj * p_)); p.fdP = make_fastdiv((uint32_t)p_); p.fdUP = make_fastdiv((uint32_t)(u * p_));
    const int64_t gz = (int64_t)B * p.Tt;
    REQUIRE(gz <= 65535 && p.h <= 65535, "sf_pixel_targets_f32: more than 65535 (sample, token frame) pairs");
    REQUIRE((int64_t)B * 3 * T * H * W < (1ll << 40), "sf_pixel_targets_f32: clip too large");
    hipLaunchKernelGGL(sf_pixel_targets_kernel, dim3(chunks, p.h, (unsigned)gz), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("pixel_targets_f32");
}


// ================================================================================================
// MoCo step glue (sf_moco.h; slowfast/models/contrastive.py: Normalize, the moco branch of forward, _dequeue_and_enqueue,
// _update_history).
extern "C" int sf_l2norm_rows(int32_t n, int32_t C, const float* x, int32_t ld, const int32_t* perm, float* out,
                              sf_stream_t stream) {
    REQUIRE(x && out, "sf_l2norm_rows: null pointer");
    REQUIRE(n > 0 && C > 0 && ld >= C, "sf_l2norm_rows: bad shape (n=%d, C=%d, ld=%d)", n, C, ld);
    L2NormParams p;
    p.x = x; p.perm = perm; p.out = out; p.n = n; p.C = C; p.ld = ld;
    hipLaunchKernelGGL(sf_l2norm_rows_kernel, dim3(cdiv(n, SF_THREADS / 64)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("l2norm_rows");
}

static int moco_slab_rows(int32_t K) {
    return SF_MOCO_CHUNK * cdiv(K, (int64_t)SF_MOCO_CHUNK * SF_MOCO_SLABS);
}
static int moco_check(const char* who, int32_t n, int32_t V, int32_t K, int32_t C) {
    REQUIRE(n > 0 && V > 0 && K >= 1, "%s: bad shape (n=%d, V=%d, K=%d)", who, n, V, K);
    REQUIRE(C > 0 && C % 64 == 0 && C <= 256, "%s: C = %d: the feature dimension must be a multiple of 64 up to 256", who, C);
    REQUIRE((int64_t)n * C <= SF_MOCO_QMAX, "%s: n * C = %lld is beyond the query rows one workgroup keeps (<= %d)", who,
            (long long)n * C, SF_MOCO_QMAX);
    REQUIRE(V <= SF_MOCO_VMAX, "%s: %d key views (<= %d)", who, V, SF_MOCO_VMAX);
    REQUIRE(((int64_t)V * n) * ((int64_t)K + 1) < (1ll << 40), "%s: logits too large", who);
    return 0;
}
extern "C" int64_t sf_moco_nce_workspace(int32_t n, int32_t V, int32_t K, int32_t C) {
    if (moco_check("sf_moco_nce_workspace", n, V, K, C)) return -1;
    const int64_t nslab = cdiv(K, moco_slab_rows(K));
    return 4 * ((nslab * n * 2 + 3) / 4 * 4 + nslab * n * C);
}
static int moco_fill(const char* who, MocoNceParams& p, int32_t n, int32_t V, int32_t K, int32_t C, const float* f,
                     const float* key, const float* queue, float inv_T, float* logits, float* df, float* loss, void* ws,
                     int64_t ws_bytes) {
    if (moco_check(who, n, V, K, C)) return -1;
    REQUIRE(f && key && queue && logits && df && loss && ws, "%s: null pointer", who);
    REQUIRE((uintptr_t)queue % 16 == 0 && (uintptr_t)ws % 16 == 0, "%s: the queue and the workspace must be 16-byte aligned", who);
    REQUIRE(ws_bytes >= sf_moco_nce_workspace(n, V, K, C), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
            (long long)sf_moco_nce_workspace(n, V, K, C));
    p.f = f; p.key = key; p.queue = queue; p.logits = logits; p.df = df; p.loss = loss;
    p.n = n; p.V = V; p.K = K; p.C = C; p.invT = inv_T;
    p.slab_rows = moco_slab_rows(K);
    p.nslab = cdiv(K, p.slab_rows);
    p.ws_ms = (float*)ws;
    p.ws_a = (float*)ws + ((int64_t)p.nslab * n * 2 + 3) / 4 * 4;
    return 0;
}
extern "C" int sf_moco_nce_slabs(int32_t n, int32_t V, int32_t K, int32_t C, const float* f, const float* key,
                                 const float* queue, float inv_T, float* logits, float* df, float* loss, void* ws,
                                 int64_t ws_bytes, sf_stream_t stream) {
    MocoNceParams p;
    if (moco_fill("sf_moco_nce_slabs", p, n, V, K, C, f, key, queue, inv_T, logits, df, loss, ws, ws_bytes)) return -1;
    const dim3 grid(p.nslab), block(SF_THREADS);
    switch (C) {
        case 64: hipLaunchKernelGGL(sf_moco_nce_slab_kernel<64>, grid, block, 0, (hipStream_t)stream, p); break;
        case 128: hipLaunchKernelGGL(sf_moco_nce_slab_kernel<128>, grid, block, 0, (hipStream_t)stream, p); break;
        case 192: hipLaunchKernelGGL(sf_moco_nce_slab_kernel<192>, grid, block, 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(sf_moco_nce_slab_kernel<256>, grid, block, 0, (hipStream_t)stream, p); break;
    }
    return check_launch("moco_nce_slabs");
}
extern "C" int sf_moco_nce_finalize(int32_t n, int32_t V, int32_t K, int32_t C, const float* f, const float* key,
                                    const float* queue, float inv_T, float* logits, float* df, float* loss, void* ws,
                                    int64_t ws_bytes, sf_stream_t stream) {
    MocoNceParams p;
    if (moco_fill("sf_moco_nce_finalize", p, n, V, K, C, f, key, queue, inv_T, logits, df, loss, ws, ws_bytes)) return -1;
    hipLaunchKernelGGL(sf_moco_nce_finalize_kernel, dim3(n + 1), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("moco_nce_finalize");
}

extern "C" int sf_queue_enqueue(int32_t K, int32_t C, int32_t rows, int32_t views, const float* keys, float* queue,
                                int64_t* ptr, int32_t* err, sf_stream_t stream) {
    REQUIRE(keys && queue && ptr && err, "sf_queue_enqueue: null pointer");
    REQUIRE(K > 0 && C > 0 && rows > 0 && views > 0, "sf_queue_enqueue: bad shape (K=%d, C=%d, rows=%d, views=%d)", K, C, rows,
            views);
    REQUIRE(K % rows == 0, "sf_queue_enqueue: K %% rows != 0 (K=%d, rows=%d): the queue length must be a multiple of the key "
            "batch", K, rows);
    EnqueueParams p;
    p.keys = keys; p.queue = queue; p.ptr = ptr; p.err = err; p.K = K; p.C = C; p.rows = rows; p.views = views;
    p.vec = C % 4 == 0 && (uintptr_t)keys % 16 == 0 && (uintptr_t)queue % 16 == 0;
    hipLaunchKernelGGL(sf_queue_enqueue_kernel, dim3(1), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("queue_enqueue");
}

extern "C" int sf_ema_update(int64_t n, const float* p_, float* hist, const float* mm, sf_stream_t stream) {
    REQUIRE(p_ && hist && mm && n > 0, "sf_ema_update: bad arguments");
    REQUIRE((uintptr_t)p_ % 4 == 0 && (uintptr_t)hist % 4 == 0, "sf_ema_update: the buffers must be 4-byte aligned");
    EmaParams p;
    p.p = p_; p.hist = hist; p.mm = mm; p.n = n;
    p.vec = (uintptr_t)p_ % 16 == 0 && (uintptr_t)hist % 16 == 0;
    hipLaunchKernelGGL(sf_ema_update_kernel, dim3(sf_flat_blocks(n)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("ema_update");
}

// ================================================================================================
// BYOL similarity loss (sf_byol.h; slowfast/models/contrastive.py: Normalize, sim_loss and the byol branch of forward).
static int byol_check(const char* who, int32_t n, int32_t V, int32_t C) {
    REQUIRE(n > 0, "%s: bad shape (n=%d)", who, n);
    REQUIRE(V >= 1 && V <= SF_BYOL_VMAX, "%s: %d key views (1 .. %d)", who, V, SF_BYOL_VMAX);
    REQUIRE(C >= 1 && C <= SF_BYOL_CMAX, "%s: C = %d: the feature dimension must be 1 .. %d", who, C, SF_BYOL_CMAX);
    return 0;
}
extern "C" int64_t sf_byol_sim_workspace(int32_t n, int32_t V, int32_t C) {
    if (byol_check("sf_byol_sim_workspace", n, V, C)) return -1;
    return 4 * (int64_t)n;
}
static int byol_fill(const char* who, ByolSimParams& p, int32_t n, int32_t V, int32_t C, const float* x, int32_t ld,
                     const float* key, float inv_T, float* df, float* loss, void* ws, int64_t ws_bytes) {
    if (byol_check(who, n, V, C)) return -1;
    REQUIRE(x && key && df && loss && ws, "%s: null pointer", who);
    REQUIRE(ld >= C, "%s: row pitch %d below C = %d", who, ld, C);
    REQUIRE(ws_bytes >= 4 * (int64_t)n, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, 4ll * n);
    p.p = x; p.key = key; p.df = df; p.loss = loss; p.ws = (float*)ws;
    p.n = n; p.V = V; p.C = C; p.ld = ld; p.invT = inv_T;
    p.coef = (float)(-(double)inv_T / ((double)V * (double)n));
    return 0;
}
extern "C" int sf_byol_sim_rows(int32_t n, int32_t V, int32_t C, const float* x, int32_t ld, const float* key, float inv_T,
                                float* df, float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream) {
    ByolSimParams p;
    if (byol_fill("sf_byol_sim_rows", p, n, V, C, x, ld, key, inv_T, df, loss, ws, ws_bytes)) return -1;
    hipLaunchKernelGGL(sf_byol_sim_rows_kernel, dim3(cdiv(n, SF_THREADS / 64)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("byol_sim_rows");
}
extern "C" int sf_byol_sim_finalize(int32_t n, int32_t V, int32_t C, const float* x, int32_t ld, const float* key, float inv_T,
                                    float* df, float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream) {
    ByolSimParams p;
    if (byol_fill("sf_byol_sim_finalize", p, n, V, C, x, ld, key, inv_T, df, loss, ws, ws_bytes)) return -1;
    hipLaunchKernelGGL(sf_byol_sim_finalize_kernel, dim3(1), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("byol_sim_finalize");
}

// ================================================================================================
// SimCLR NT-Xent loss (sf_simclr.h; slowfast/models/contrastive.py: Normalize and the simclr branch of forward).
static int simclr_check(const char* who, int32_t n, int32_t C) {
    REQUIRE(n >= 1 && n <= SF_SIMCLR_NMAX, "%s: n = %d: the rows per crop must be 1 .. %d", who, n, SF_SIMCLR_NMAX);
    REQUIRE(C >= 1 && C <= SF_SIMCLR_CMAX, "%s: C = %d: the feature dimension must be 1 .. %d", who, C, SF_SIMCLR_CMAX);
    return 0;
}
static int64_t simclr_pad4(int64_t x) { return (x + 3) / 4 * 4; }
extern "C" int64_t sf_simclr_workspace(int32_t n, int32_t C) {
    if (simclr_check("sf_simclr_workspace", n, C)) return -1;
    const int64_t M = 2 * (int64_t)n;
    return 4 * (simclr_pad4(M * C) + 3 * simclr_pad4(M) + M * M);       // q, |x|, D, the row terms, E
}
static int simclr_fill(const char* who, SimclrParams& p, int32_t n, int32_t C, const float* a, int32_t lda, const float* b,
                       int32_t ldb, float inv_T, float* da, float* db, float* loss, float* q_out, void* ws, int64_t ws_bytes) {
    if (simclr_check(who, n, C)) return -1;
    REQUIRE(a && b && da && db && loss && ws, "%s: null pointer", who);
    REQUIRE(lda >= C && ldb >= C, "%s: row pitches %d, %d below C = %d", who, lda, ldb, C);
    REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", who);
    REQUIRE(ws_bytes >= sf_simclr_workspace(n, C), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
            (long long)sf_simclr_workspace(n, C));
    const int64_t M = 2 * (int64_t)n;
    p.a = a; p.b = b; p.da = da; p.db = db; p.loss = loss; p.q_out = q_out;
    p.q = (float*)ws;
    p.nrm = p.q + simclr_pad4(M * C);
    p.D = p.nrm + simclr_pad4(M);
    p.term = p.D + simclr_pad4(M);
    p.E = p.term + simclr_pad4(M);
    p.n = n; p.M = (int)M; p.C = C; p.lda = lda; p.ldb = ldb;
    p.cw = C <= 64 ? 64 : (C <= 128 ? 128 : SF_THREADS);
    p.ktiles = cdiv((int)M, SF_SIMCLR_RK * (SF_THREADS / p.cw));
    p.invT = inv_T;
    p.coef = (float)((double)inv_T / (double)M);
    return 0;
}
#define SF_SIMCLR_ARGS int32_t n, int32_t C, const float* a, int32_t lda, const float* b, int32_t ldb, float inv_T, float* da, \
                       float* db, float* loss, float* q_out, void* ws, int64_t ws_bytes, sf_stream_t stream
#define SF_SIMCLR_FILL(who) \
    SimclrParams p;         \
    if (simclr_fill(who, p, n, C, a, lda, b, ldb, inv_T, da, db, loss, q_out, ws, ws_bytes)) return -1
extern "C" int sf_simclr_norm(SF_SIMCLR_ARGS) {
    SF_SIMCLR_FILL("sf_simclr_norm");
    hipLaunchKernelGGL(sf_simclr_norm_kernel, dim3(cdiv(p.M, SF_THREADS / 64)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("simclr_norm");
}
extern "C" int sf_simclr_rows(SF_SIMCLR_ARGS) {
    SF_SIMCLR_FILL("sf_simclr_rows");
    hipLaunchKernelGGL(sf_simclr_rows_kernel, dim3(cdiv(p.M, SF_SIMCLR_TI)), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("simclr_rows");
}
extern "C" int sf_simclr_grad(SF_SIMCLR_ARGS) {
    SF_SIMCLR_FILL("sf_simclr_grad");
    hipLaunchKernelGGL(sf_simclr_grad_kernel, dim3(p.ktiles + 1), dim3(SF_THREADS), 0, (hipStream_t)stream, p);
    return check_launch("simclr_grad");
}
