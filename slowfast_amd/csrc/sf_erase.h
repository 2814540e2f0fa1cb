// Random erasing of a training batch on the device (slowfast/datasets/random_erasing.py; datasets/kinetics.py:437-447 erases
// the normalised fp32 clip on the host just before pack_pathway_output).  The draw stays on the host
// (slowfast_amd/random_erasing.py) and arrives as ONE table; the two streaming kernels of sf_erase_clip_f32 apply it to a dense fp32 (N, C, T, H, W) batch: in place
// (only erased elements are written, nothing is read), or into another buffer (every element read once and written once).
//
// The packed uint8 path (sf_pack_clip_u8_aug and sf_pack_clip_u8_sample, sf_pack.h) erases with erase_find() and erase_value1()
// of this file, in fp32 between the normalisation and the mixing.
//
// The table (int32 words, one host-to-device copy):  R rows of SF_ERASE_ROW_WORDS words
//     [0] n  [1] t0  [2] t1  [3] top  [4] left  [5] h  [6] w  [7] key_lo  [8] key_hi  [9] colour word offset  [10] end  [11] 0
// in draw order with the rows of one sample adjacent and samples ascending, then N + 1 words first_row[n] (rows of sample n
// are first_row[n] .. first_row[n + 1] - 1; `end` of a row is first_row[n + 1]), then the `rand`-mode colours as float bits:
// row r owns (t1 - t0) * C floats at its colour offset, indexed (t - t0) * C + c.
//
// Overlap.  The reference assigns the boxes of a sample one after the other, so the LAST row that contains an element decides
// its value.  No kernel relies on store order for that: the in-place kernel gives every row its own slice of the grid and a
// thread skips an element that a later row of the same sample contains (that row's slice writes it), the copy kernel and
// the packed path search the sample's rows from the last one down.  Every erased element is therefore stored exactly once.
//
// Element identity.  A value depends on (row, c, t, y, x) of the NORMALISED clip only: idx = ((c * T + t) * H + y) * W + x
// with t the source frame and c the channel in DATA.MEAN order -- before pathway selection and channel reversal, so the Slow
// pathway is the index_select of the Fast one bit for bit and REVERSE_INPUT_CHANNEL permutes the noise with the image.
//
// `pixel` noise.  Philox4x32-10, key = the row's 64-bit key, counter = (g, 0, 0, 0) with g = idx >> 2; the four outputs
// r0..r3 serve elements 4g..4g+3:  u = r * 2^-32 + 2^-33 (fp32),  rad = sqrtf(-2 * logf(u_a)),  ang = fl(2 pi) * u_b,
// z_even = rad * sinf(ang),  z_odd = rad * cosf(ang), with (u_a, u_b) = (u(r0), u(r1)) for elements 0 / 1 of the group and
// (u(r2), u(r3)) for elements 2 / 3.  The integer stream is exact everywhere; only logf / sinf / cosf differ in the last bits
// between the device, the host simulator and the float64 restatement of the tests.
#pragma once
#include "sf_common.h"

#define SF_ERASE_ROW_WORDS 12
enum { SF_ERASE_CONST = 0, SF_ERASE_RAND = 1, SF_ERASE_PIXEL = 2 };

struct EraseRow {
    int n, t0, t1, top, left, h, w;
    uint32_t key_lo, key_hi;
    int col, end;
};
__device__ __forceinline__ EraseRow erase_row(const int* tab, int r) {
    const int* p = tab + (int64_t)r * SF_ERASE_ROW_WORDS;
    EraseRow e;
    e.n = p[0]; e.t0 = p[1]; e.t1 = p[2]; e.top = p[3]; e.left = p[4]; e.h = p[5]; e.w = p[6];
    e.key_lo = (uint32_t)p[7]; e.key_hi = (uint32_t)p[8]; e.col = p[9]; e.end = p[10];
    return e;
}
__device__ __forceinline__ bool erase_row_has(const int* tab, int r, int t, int y, int x) {
    const int* p = tab + (int64_t)r * SF_ERASE_ROW_WORDS;
    return t >= p[1] && t < p[2] && (unsigned)(y - p[3]) < (unsigned)p[5] && (unsigned)(x - p[4]) < (unsigned)p[6];
}
// the row that decides element (t, y, x) of sample n: the last one that contains it, -1 when none does
__device__ __forceinline__ int erase_find(const int* tab, const int* first_row, int n, int t, int y, int x) {
    const int lo = first_row[n];
    for (int r = first_row[n + 1] - 1; r >= lo; --r)
        if (erase_row_has(tab, r, t, y, x)) return r;
    return -1;
}

// ---- Philox4x32-10 (Salmon et al., SC'11) --------------------------------------------------------------------------
struct Philox4 { uint32_t v[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
__device__ __forceinline__ float erase_uniform(uint32_t r) { return (float)r * 0x1p-32f + 0x1p-33f; }
// Box-Muller on one pair of outputs: (z_even, z_odd)
__device__ __forceinline__ void erase_normal_pair(uint32_t ra, uint32_t rb, float& z_even, float& z_odd) {
    const float rad = sqrtf(-2.0f * logf(erase_uniform(ra)));
    const float ang = 6.28318530717958647692f * erase_uniform(rb);
    z_even = rad * sinf(ang);
    z_odd = rad * cosf(ang);
}
// the four normals of group g (elements 4g .. 4g+3) under a row's key
__device__ __forceinline__ f32x4 erase_noise4(uint32_t key_lo, uint32_t key_hi, uint64_t g) {
    const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, key_lo, key_hi);
    f32x4 z;
    float a, b;
    erase_normal_pair(r.v[0], r.v[1], a, b); z[0] = a; z[1] = b;
    erase_normal_pair(r.v[2], r.v[3], a, b); z[2] = a; z[3] = b;
    return z;
}
// one element (the packed kernel's threads own one pixel each): only the pair that holds it is transformed
__device__ __forceinline__ float erase_noise1(uint32_t key_lo, uint32_t key_hi, uint64_t idx) {
    const uint64_t g = idx >> 2;
    const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, key_lo, key_hi);
    const int e = (int)(idx & 3);
    float a, b;                                             // selects, not r.v[e & 2]: a runtime index would move r into LDS
    erase_normal_pair((e & 2) ? r.v[2] : r.v[0], (e & 2) ? r.v[3] : r.v[1], a, b);
    return (e & 1) ? b : a;
}
// value of element (c, t, idx) under row r (row words at p)
__device__ __forceinline__ float erase_value1(const int* tab, int r, int mode, int C, int c, int t, uint64_t idx) {
    const int* p = tab + (int64_t)r * SF_ERASE_ROW_WORDS;
    if (mode == SF_ERASE_PIXEL) return erase_noise1((uint32_t)p[7], (uint32_t)p[8], idx);
    if (mode == SF_ERASE_RAND) return reinterpret_cast<const float*>(tab)[p[9] + (t - p[1]) * C + c];
    return 0.0f;
}

struct EraseClipParams {
    const float* src;
    float* dst;
    const int* tab;             // device copy of the table
    const int* first_row;       // tab + R * SF_ERASE_ROW_WORDS
    int N, C, T, H, W, mode;
    int64_t S;                  // elements per sample (< 2^31)
    int64_t items;              // copy kernel: 4-element groups per sample
};

// ------------------------------------------------------------------------------------------------
// in place: grid.y = table row, grid.x strides over the row's work items.  One item = one Philox group (elements 4g..4g+3 of
// the sample, g = idx >> 2) of one box row (c, t, y): item -> (plane, yy, gi) with gi < ng = (w + 2) / 4 + 1, the most groups
// w consecutive elements can touch; a box row that touches fewer skips the surplus.  A group that lies wholly inside the box
// row, is owned by this table row (no later row of the sample contains any of its elements) and is 16-byte aligned is one
// 16-byte store; at the box edges, under a partial overlap and in a sample whose base is not 16-byte aligned the owned
// elements go as aligned 8-byte pairs where two neighbours allow it and as single dwords otherwise.  Nothing is loaded from
// the clip.
__global__ __launch_bounds__(SF_THREADS) void sf_erase_inplace_kernel(EraseClipParams p) {
    const int r = blockIdx.y;
    const EraseRow e = erase_row(p.tab, r);
    const int ng = (e.w + 2) / 4 + 1;
    const int frames = e.t1 - e.t0;
    const uint32_t items = (uint32_t)((int64_t)p.C * frames * e.h * ng);         // <= 2 * S < 2^32 (checked on the host)
    float* out = p.dst + (int64_t)e.n * p.S;
    const bool base16 = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const bool base8 = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    const float* colours = reinterpret_cast<const float*>(p.tab);
    for (uint32_t it = blockIdx.x * SF_THREADS + threadIdx.x; it < items; it += gridDim.x * SF_THREADS) {
        const int gi = (int)(it % (uint32_t)ng);
        uint32_t q = it / (uint32_t)ng;
        const int yy = (int)(q % (uint32_t)e.h); q /= (uint32_t)e.h;
        const int tt = (int)(q % (uint32_t)frames);
        const int c = (int)(q / (uint32_t)frames);
        const int t = e.t0 + tt, y = e.top + yy;
        const int64_t line = (((int64_t)c * p.T + t) * p.H + y) * p.W;     // idx of (c, t, y, 0)
        const int64_t i0 = line + e.left, i1 = i0 + e.w;                 // the box row: idx in [i0, i1)
        const int64_t g = (i0 >> 2) + gi;
        if (g * 4 >= i1) continue;
        unsigned own = 0;                                                // bit k: element 4g + k is written by this row
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t idx = g * 4 + k;
            if (idx < i0 || idx >= i1) continue;
            const int x = (int)(idx - line);
            bool later = false;
            for (int r2 = r + 1; r2 < e.end; ++r2) later = later || erase_row_has(p.tab, r2, t, y, x);
            if (!later) own |= 1u << k;
        }
        if (own == 0) continue;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.mode == SF_ERASE_PIXEL) v = erase_noise4(e.key_lo, e.key_hi, (uint64_t)g);
        else if (p.mode == SF_ERASE_RAND) { const float col = colours[e.col + tt * p.C + c]; v[0] = v[1] = v[2] = v[3] = col; }
        float* o = out + g * 4;
        if (own == 0xFu && base16) {
            *reinterpret_cast<f32x4*>(o) = v;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
            const unsigned pair = (own >> k) & 3u;
            if (pair == 3u && base8) {
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                f32x2 w2 = {v[k], v[k + 1]};
                *reinterpret_cast<f32x2*>(o + k) = w2;
            } else {
                if (pair & 1u) o[k] = v[k];
                if (pair & 2u) o[k + 1] = v[k + 1];
            }
        }
    }
}

// into another buffer: grid.y = sample, one item = 4 consecutive elements of the sample (the Philox group when it is needed);
// dst = the deciding row's value where a row contains the element, src otherwise.  16-byte accesses when both sample bases
// are 16-byte aligned, element by element otherwise and in the tail of a sample whose size is no multiple of 4.
__global__ __launch_bounds__(SF_THREADS) void sf_erase_copy_kernel(EraseClipParams p) {
    const int n = blockIdx.y;
    const float* in = p.src + (int64_t)n * p.S;
    float* out = p.dst + (int64_t)n * p.S;
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const bool any = p.first_row[n + 1] > p.first_row[n];
    const int HW = p.H * p.W;
    for (int64_t g = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; g < p.items; g += (int64_t)gridDim.x * SF_THREADS) {
        const int64_t base = g * 4;
        const int cnt = p.S - base < 4 ? (int)(p.S - base) : 4;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec && cnt == 4) v = *reinterpret_cast<const f32x4*>(in + base);
        else for (int k = 0; k < cnt; ++k) v[k] = in[base + k];
        if (any) {
            int rows[4] = {-1, -1, -1, -1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= cnt) continue;
                const uint32_t idx = (uint32_t)base + k;
                const uint32_t plane = idx / (uint32_t)HW, rem = idx - plane * (uint32_t)HW;
                rows[k] = erase_find(p.tab, p.first_row, n, (int)(plane % (uint32_t)p.T), (int)(rem / (uint32_t)p.W),
                                     (int)(rem % (uint32_t)p.W));
            }
            if (p.mode == SF_ERASE_PIXEL && rows[0] >= 0 && rows[0] == rows[1] && rows[0] == rows[2] && rows[0] == rows[3]) {
                const int* rp = p.tab + (int64_t)rows[0] * SF_ERASE_ROW_WORDS;     // the common case inside a box: one Philox call
                v = erase_noise4((uint32_t)rp[7], (uint32_t)rp[8], (uint64_t)g);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (rows[k] < 0) continue;
                    const uint32_t idx = (uint32_t)base + k;
                    const uint32_t plane = idx / (uint32_t)HW;
                    v[k] = erase_value1(p.tab, rows[k], p.mode, p.C, (int)(plane / (uint32_t)p.T), (int)(plane % (uint32_t)p.T),
                                        (uint64_t)idx);
                }
            }
        }
        if (vec && cnt == 4) *reinterpret_cast<f32x4*>(out + base) = v;
        else for (int k = 0; k < cnt; ++k) out[base + k] = v[k];
    }
}
