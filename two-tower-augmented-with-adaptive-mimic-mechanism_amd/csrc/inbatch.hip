// In-batch negatives (ttamm's in-batch mode, BASELINE configs C2/C4; definition in
// oracle/cpu_reference.py train_step(in_batch=True) — not reference behaviour, which scores
// sampled negatives only, training.py:770-798):
//
//   S  = U P^T              [B, Bc]  users x every positive of the (global) batch, fp32-accurate MFMA
//   dS = (sigmoid(S) - Y) / T        Y(b, j) = (j == row_base + b), T = logits in the BCE mean
//   dU = dS P   [B, D]               dP = dS^T U   [Bc, D]        + the BCE sum of S
//
// Nothing B x Bc is stored.  One launch holds two roles over the same code: "user" blocks own
// 128 user rows and a split of the columns (items) and accumulate dU; "item" blocks own 128
// positive rows and a split of the users and accumulate dP, recomputing S^T.  A block's 4 waves
// each keep their 32 rows' operand fragments in registers for the whole launch; the column
// operand streams through LDS in 64-row tiles (double buffered).  Per tile a wave computes its
// 32 x 64 score block (v_mfma_f32_32x32x2_f32, K = D), turns it into dS in registers, parks dS in
// its LDS slice and multiplies it back against the same LDS tile (K = 64).  Blocks write
// partial rows to slabs that ib_reduce_kernel sums in split order (deterministic).  This fp32-MFMA
// kernel runs with TTAMM_FP32_MFMA=exact; the default is the split-bf16 inbatch_x_kernel below.
//
// The softmax objective (ttamm.h in_batch_loss, ttamm_inbatch_softmax): the cross-entropy over each
// user's row of S / temperature, in two passes — inbatch_loss_kernel's softmax form (row
// log-sum-exp per column split) and ib_lse_merge_kernel own lse, the loss and the rows'
// (maximum, 1 / sum), then inbatch_x_kernel's softmax instantiation forms
// dS = (exp(S / t - max) / sum - Y) inv_count / t = (exp(S / t - lse) - Y) inv_count / t.  Only
// inbatch_x_kernel has a softmax form: under softmax launch_inbatch_softmax ignores
// TTAMM_FP32_MFMA=exact (as the forward-only BCE op does).
//
// The split-bf16 kernels (inbatch_x_kernel, inbatch_loss_kernel) are built from one set of pieces:
// ibx_row_frags (a lane's row operand), IbxStage (global -> registers -> the LDS tile image),
// ibx_score (a 32 x 32 score block) and the ibx_exp_nabs / ibx_sigmoid / ibx_bce_* element
// arithmetic, so the training and the validation BCE of a batch are one function of the same rows.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "kernels.h"

namespace ttamm {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kIbRows = 128;  // rows per block (4 waves x 32)
constexpr int kIbTile = 64;   // column tile
constexpr int kIbDsLd = kIbTile + 4;

__device__ __forceinline__ float ib_bce(float x, float y) {  // ATen BCEWithLogits term (rows.hip bce_logit)
    const float m = fmaxf(-x, 0.f);
    return (1.0f - y) * x + m + logf(expf(-m) + expf(-x - m));
}
__device__ __forceinline__ float f4at(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

template <int DP>
__global__ __launch_bounds__(256) void inbatch_kernel(InBatchArgs A) {
    constexpr int NB = DP / 32;   // 32-wide output column blocks
    constexpr int G = DP / 8;     // k groups of the score product (a lane reads 4 of each 8)
    constexpr int SD = DP + 4;    // LDS row stride of the column tile
    constexpr int TF4 = kIbTile * DP / 4;
    constexpr int LOADS = (TF4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float ct[2][kIbTile * SD];
    __shared__ __attribute__((aligned(16))) float dsb[4][32 * kIbDsLd];
    __shared__ float red[4];

    int blk = blockIdx.x;
    const int nu = A.rblk_u * A.splits_u;
    const bool role_u = blk < nu;
    if (!role_u) blk -= nu;
    const int splits = role_u ? A.splits_u : A.splits_p;
    const int rb = blk / splits, sp = blk - (blk / splits) * splits;
    const float* R = role_u ? A.U : A.P;
    const int64_t ldr = role_u ? A.ldu : A.ldp, nr = role_u ? A.B : A.Bc;
    const float* C = role_u ? A.P : A.U;
    const int64_t ldc = role_u ? A.ldp : A.ldu, nc = role_u ? A.Bc : A.B;
    const int64_t per = role_u ? A.cols_u : A.cols_p;
    const int64_t c_begin = min(nc, (int64_t)sp * per), c_end = min(nc, c_begin + per);
    const int D = A.D;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)rb * kIbRows + 32 * w;

    // this lane's row fragments: R[r0 + li][8g + 4h .. +3], zero past D / nr
    float4 rf[G];
    {
        const int64_t row = r0 + li;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int col = 8 * g + 4 * h;
            rf[g] = (row < nr && col < D) ? *reinterpret_cast<const float4*>(R + row * ldr + col)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    f32x16 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    float bce = 0.f;

    // column tile -> registers (zero past c_end / D, so masked rows contribute exact zeros)
    float4 st[LOADS];
    auto load = [&](int64_t c0) {
#pragma unroll
        for (int it = 0; it < LOADS; ++it) {
            const int lin = tid + it * 256;
            const int row = lin / (DP / 4), col = (lin - row * (DP / 4)) * 4;
            const int64_t gc = c0 + row;
            st[it] = (lin < TF4 && gc < c_end && col < D) ? *reinterpret_cast<const float4*>(C + gc * ldc + col)
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int it = 0; it < LOADS; ++it) {
            const int lin = tid + it * 256;
            if (lin >= TF4) continue;
            const int row = lin / (DP / 4), col = (lin - row * (DP / 4)) * 4;
            *reinterpret_cast<float4*>(&ct[buf][row * SD + col]) = st[it];
        }
    };

    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin + kIbTile - 1) / kIbTile) : 0;
    if (ntiles > 0) {
        load(c_begin);
        store(0);
    }
    __syncthreads();
    float* my_ds = dsb[w];
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const int64_t c0 = c_begin + (int64_t)t * kIbTile;
        if (t + 1 < ntiles) load(c0 + kIbTile);  // in flight during this tile's MFMAs
        const float* tile = ct[buf];
        // ---- S block: 32 rows x 64 columns, K = DP --------------------------------------------
        f32x16 s[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[j][r] = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 b = *reinterpret_cast<const float4*>(tile + (32 * j + li) * SD + 8 * g + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    s[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4at(rf[g], q), f4at(b, q), s[j], 0, 0, 0);
            }
        }
        // ---- dS in registers -> this wave's LDS slice ------------------------------------------
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int64_t gr = r0 + lr, gc = c0 + 32 * j + li;
                const bool ok = gr < nr && gc < c_end;
                const int64_t gu = role_u ? gr : gc, gi = role_u ? gc : gr;  // user row, positive column
                const float y = (gi == A.row_base + gu) ? 1.0f : 0.0f;
                const float x = s[j][r];
                const float d = ok ? (1.0f / (1.0f + expf(-x)) - y) * A.inv_T : 0.f;
                if (role_u && ok) bce += ib_bce(x, y);
                my_ds[lr * kIbDsLd + 32 * j + li] = d;
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the slice is written
        __builtin_amdgcn_wave_barrier();
        // ---- rows' gradient += dS . tile, K = 64 -----------------------------------------------
#pragma unroll
        for (int g = 0; g < kIbTile / 8; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(my_ds + li * kIbDsLd + 8 * g + 4 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float* brow = tile + (8 * g + 4 * h + q) * SD + li;
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4at(a, q), brow[32 * n], acc[n], 0, 0, 0);
            }
        }
        // the other buffer was last read in tile t - 1, before that tile's barrier
        if (t + 1 < ntiles) store(buf ^ 1);
        __syncthreads();
    }
    // ---- partial rows -> this split's slab ------------------------------------------------------
    float* slab = role_u ? A.slab_u + (int64_t)sp * A.B * D : A.slab_p + (int64_t)sp * A.Bc * D;
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t gr = r0 + lr;
            const int col = 32 * n + li;
            if (gr < nr && col < D) slab[gr * D + col] = acc[n][r];
        }
    if (role_u) {
        bce = wave_sum(bce);
        if (lane == 0) red[w] = bce;
        __syncthreads();
        if (tid == 0) A.loss_part[blk] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// ---- split-bf16 variant (default) ---------------------------------------------------------------
// The same roles, splits and slabs, on v_mfma_f32_32x32x16_bf16: every fp32 operand x is split
// into bf16 planes hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (RNE, exact
// differences) and a product is formed by six MFMAs (hh, hm, mh, hl, lh, mm; the dropped terms
// are below 2^-24 relative), as in gemm.hip's split kernel: fp32-accurate at 6/16 of the fp32
// MFMA's cycles.
//   Product 1 (per wave, per 64-column tile): S^T[c][u] = C_tile[c][:] . R[u][:]  — the tile as
//     the A operand (row reads), the wave's 32 rows as the B operand (register fragments).  S^T
//     lands with the row u on the lane and the tile column c in registers.
//   dS^T = (sigmoid(S^T) - Y) / T in registers.
//   Product 2: dR[u][:] += sum_c dS^T[c][u] . C_tile[c][:] — dS^T is the A operand straight from
//     its accumulator registers (a 32x32x16 MFMA summing over the accumulator's row index takes
//     it with no lane movement; k order 16s + 8(j>>2) + 4h + (j&3)), the tile the B operand read
//     column-wise with ds_read_b64_tr_b16 in that k order.
// The tile's three planes share one LDS image that serves both the row reads (ds_read_b128) and
// the transposed reads: 256-B rows (128 bf16, columns past D zero and never multiplied) with the
// 16-B chunks XOR-permuted by the row, conflict-free for both.  Single LDS buffer, the next tile
// in flight in registers; two blocks per CU.
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4e_t __attribute__((ext_vector_type(4)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;

constexpr int kIbxRowBytes = 256;                  // LDS image row: 128 bf16
constexpr int kIbxPlane = kIbTile * kIbxRowBytes;  // one plane of a 64-row tile

__device__ __forceinline__ int ibx_off(int row, int ch) {  // byte offset of 16-B chunk ch of row
    return row * kIbxRowBytes + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
// x -> hi, mid, lo (4 bf16 each)
__device__ __forceinline__ void ibx_split(float4 v, uint2 out[3]) {
    const f32x4e_t x = {v.x, v.y, v.z, v.w};
    const bf16x4_t h = __builtin_convertvector(x, bf16x4_t);
    const f32x4e_t r = x - __builtin_convertvector(h, f32x4e_t);
    const bf16x4_t m = __builtin_convertvector(r, bf16x4_t);
    const f32x4e_t r2 = r - __builtin_convertvector(m, f32x4e_t);
    out[0] = __builtin_bit_cast(uint2, h);
    out[1] = __builtin_bit_cast(uint2, m);
    out[2] = __builtin_bit_cast(uint2, __builtin_convertvector(r2, bf16x4_t));
}
__device__ __forceinline__ bf16x8_t ibx_cat(uint2 a, uint2 b) {
    return __builtin_bit_cast(bf16x8_t, uint4{a.x, a.y, b.x, b.y});
}
// bf16 partial products per fp32 product: 5 (hh, hm, mh, hl, lh; round 6, the default) or, in
// developer measurement builds, 6 (+ mm), 4 (hh hm mh mm) or 3 (hh hm mh).  Measured against the
// chunked float64 definition at the C4 rank-of-8 shape (profiles/r06_inbatch_products.txt):
// 6: dU 9.8e-7, dP 2.9e-6, 3.24 ms; 5: 9.7e-7, 2.9e-6, 2.97 ms; 4: 5.6e-6, 7.3e-6, 2.27 ms;
// 3: 5.7e-6, 7.0e-6, 2.00 ms (bound 1e-5) — mm (<= 2^-18 relative) is below the fp32 noise,
// hl / lh (<= 2^-17 each) are not, so 5 keeps the 6-product accuracy
#ifndef TTAMM_IB_PRODUCTS
#define TTAMM_IB_PRODUCTS 5
#endif
template <int NP = TTAMM_IB_PRODUCTS>
__device__ __forceinline__ f32x16 ibx_mfma6(const bf16x8_t a[3], const bf16x8_t b[3], f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    if constexpr (NP == 6 || NP == 5) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    }
    if constexpr (NP == 6 || NP == 4)
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    return c;
}
// The softmax instantiations (the LSE pass, both products of the gradient kernel) keep all 6: a
// row's gradient is dominated by its own positive's term instead of averaging over the row, and
// the logit error is multiplied by 1 / temperature in the exponent, so mm (<= 2^-18 relative)
// shows.  Against the float64 definition (profiles/inbatch_softmax_products.txt), 5 -> 6 products:
// t = 1, 300 x 300 x 96: dU 7.7e-6 -> 4.5e-7, dP 6.8e-6 -> 4.8e-7; t = 0.25: dP 1.0e-5 -> 3.1e-6;
// t = 0.02 (200 x 900 x 64): dU 5.8e-5 -> 5.9e-6 (float32 torch: 7.5e-6), for 1.18x -> 1.31x the BCE
// op's time at 8192 x 8192 x 96.  The sixth product in the score product of the gradient kernel
// alone is worse than none (t = 0.25: 3.4e-5): p = exp(z - lse) needs z and lse from one S.
#ifndef TTAMM_IB_SOFTMAX_PRODUCTS
#define TTAMM_IB_SOFTMAX_PRODUCTS 6
#endif
// partial products of a kernel's LOSS form
template <int LOSS>
constexpr int kIbxProducts = LOSS == TTAMM_INBATCH_SOFTMAX ? TTAMM_IB_SOFTMAX_PRODUCTS : TTAMM_IB_PRODUCTS;

// ---- the pieces both split-bf16 kernels are made of ------------------------------------------------
// A lane's row fragments (B operand of product 1) of half wave h: row[16 s + 8 h + j] in the three
// planes, zero past D and where the row is past the operand's last (!row_ok: row is not read).
template <int KS>
__device__ __forceinline__ void ibx_row_frags(const float* row, bool row_ok, int D, int h, bf16x8_t (&rf)[KS][3]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * h;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = (row_ok && col < D) ? *reinterpret_cast<const float4*>(row + col) : z;
        const float4 b = (row_ok && col + 4 < D) ? *reinterpret_cast<const float4*>(row + col + 4) : z;
        uint2 pa[3], pb[3];
        ibx_split(a, pa);
        ibx_split(b, pb);
#pragma unroll
        for (int q = 0; q < 3; ++q) rf[s][q] = ibx_cat(pa[q], pb[q]);
    }
}

// A 64-row column tile on its way into LDS, staged by a block of NT threads (this one is tid) from
// the rows of C below c_end: load() takes rows c0 .. c0 + 63 into registers (zero past c_end / D, so
// masked rows contribute exact zeros), store() splits them into the three planes of the LDS image
// at dst.
template <int DP, int NT>
struct IbxStage {
    static constexpr int TF4 = kIbTile * DP / 4;  // float4 per column tile
    static constexpr int LOADS = TF4 / NT;
    static_assert(TF4 % NT == 0, "whole staging rounds");
    const float* C;
    int64_t ldc, c_end;
    int D, tid;
    float4 st[LOADS];

    __device__ __forceinline__ void load(int64_t c0) {
#pragma unroll
        for (int it = 0; it < LOADS; ++it) {
            const int lin = tid + it * NT;
            const int row = lin / (DP / 4), col = (lin - row * (DP / 4)) * 4;
            const int64_t gc = c0 + row;
            st[it] = (gc < c_end && col < D) ? *reinterpret_cast<const float4*>(C + gc * ldc + col)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ void store(unsigned char* dst) const {
#pragma unroll
        for (int it = 0; it < LOADS; ++it) {
            const int lin = tid + it * NT;
            const int row = lin / (DP / 4), c4 = lin - row * (DP / 4);
            const int o = ibx_off(row, c4 >> 1) + 8 * (c4 & 1);
            uint2 pl[3];
            ibx_split(st[it], pl);
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(dst + q * kIbxPlane + o) = pl[q];
        }
    }
};

// Product 1: the S^T block [32 c x 32 u] of tile rows 32 jc .. 32 jc + 31 against the wave's rows
// (lane: row u = li of half wave h; register r: tile column 32 jc + (r & 3) + 8 (r >> 2) + 4 h).
template <int NP, int KS>
__device__ __forceinline__ f32x16 ibx_score(const unsigned char* tile, int jc, int li, int h,
                                            const bf16x8_t (&rf)[KS][3]) {
    f32x16 s2;
#pragma unroll
    for (int r = 0; r < 16; ++r) s2[r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int o = ibx_off(32 * jc + li, 2 * s + h);
        bf16x8_t a[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const bf16x8_t*>(tile + q * kIbxPlane + o);
        s2 = ibx_mfma6<NP>(a, rf[s], s2);
    }
    return s2;
}

// The element arithmetic on hardware exp2 / log2 / rcp (<= 1-2 ulp): the elementwise pass, not the
// MFMAs, bounds the kernels with IEEE expf / logf / division.  Sigmoid and the ATen BCE term from
// one exp: t = exp(-|x|); for x >= 0 exp(-max(-x,0)) = 1 and exp(-x-max(-x,0)) = t, for x < 0 the
// reverse.
__device__ __forceinline__ float ibx_exp_nabs(float x) { return __builtin_amdgcn_exp2f(-fabsf(x) * 1.4426950408889634f); }
__device__ __forceinline__ float ibx_sigmoid(float x, float t) {
    const float inv = __builtin_amdgcn_rcpf(1.0f + t);
    return x >= 0.f ? inv : t * inv;
}
// label-free (y = 0): the term is max(x, 0) + ln(1 + t) (x + max(-x, 0) == max(x, 0) exactly), kept
// as two lane sums (the log2 terms are scaled by ln 2 once at the end)
__device__ __forceinline__ void ibx_bce_free(float x, float t, float& lin, float& lg2) {
    lin += fmaxf(x, 0.f);
    lg2 += __builtin_amdgcn_logf(1.0f + t);
}
// the term under label y
__device__ __forceinline__ float ibx_bce_term(float x, float y, float t) {
    return (1.0f - y) * x + fmaxf(-x, 0.f) + __builtin_amdgcn_logf(1.0f + t) * 0.6931471805599453f;
}

// 4 waves (32 rows each), two blocks per CU.
// LOSS (compile time; the BCE code is the same with or without the softmax branch):
//   TTAMM_INBATCH_BCE      dS = (sigmoid(S) - Y) * inv_T, the BCE terms summed into loss_part;
//   TTAMM_INBATCH_SOFTMAX  dS = (exp2(S * z_scale - rmax) * rinv - Y) * inv_T with the rows' (rmax,
//     rinv) = (maximum, 1 / sum; log2 units) from the LSE pass: the user role keeps its row's pair in
//     two registers, the item role (register index = user) stages the tile's 64 users' pairs next
//     to the tile and reads them as float4 (registers r & 3 of one r >> 2 group are four
//     consecutive tile columns; every lane of a half wave reads one address: a broadcast).  inv_T
//     multiplies the accumulators once at the slab write, not every element.  No loss is
//     accumulated: the LSE pass owns it.
template <int DP, int LOSS = TTAMM_INBATCH_BCE>
__global__ __launch_bounds__(2 * kIbRows, 2) void inbatch_x_kernel(InBatchArgs A) {
    constexpr int NW = kIbRows / 32;                 // waves
    constexpr int NT = 64 * NW;                      // threads
    constexpr int NB = DP / 32;                      // 32-wide output column blocks
    constexpr int KS = DP / 16;                      // k steps of product 1
    constexpr bool SOFTMAX = LOSS == TTAMM_INBATCH_SOFTMAX;
    constexpr int NP = kIbxProducts<LOSS>;
    static_assert(NT >= 2 * kIbTile, "one thread per staged rmax / rinv");
    __shared__ __attribute__((aligned(16))) unsigned char tile[3 * kIbxPlane];
    __shared__ float red[NW];
    // [rmax | rinv][tile column]
    __shared__ __attribute__((aligned(16))) float nrm_t[2][SOFTMAX ? kIbTile : 2];

    int blk = blockIdx.x;
    const int nu = A.rblk_u * A.splits_u;
    const bool role_u = blk < nu;
    if (!role_u) blk -= nu;
    const int splits = role_u ? A.splits_u : A.splits_p;
    const int rb = blk / splits, sp = blk - (blk / splits) * splits;
    const float* R = role_u ? A.U : A.P;
    const int64_t ldr = role_u ? A.ldu : A.ldp, nr = role_u ? A.B : A.Bc;
    const float* C = role_u ? A.P : A.U;
    const int64_t ldc = role_u ? A.ldp : A.ldu, nc = role_u ? A.Bc : A.B;
    const int64_t per = role_u ? A.cols_u : A.cols_p;
    const int64_t c_begin = min(nc, (int64_t)sp * per), c_end = min(nc, c_begin + per);
    const int D = A.D;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)rb * kIbRows + 32 * w;

    bf16x8_t rf[KS][3];
    ibx_row_frags(R + (r0 + li) * ldr, r0 + li < nr, D, h, rf);
    f32x16 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    float bce = 0.f, bce_lin = 0.f, bce_log2 = 0.f;

    IbxStage<DP, NT> stage{C, ldc, c_end, D, tid};
    // softmax: the user role's row (rmax, rinv) in two registers; the item role's tile columns are
    // users, whose pairs travel with the tile (threads 0..63 rmax, 64..127 rinv; zero past c_end:
    // those elements are masked)
    const int64_t gr = r0 + li;
    float max_r = 0.f, inv_r = 0.f, st_l = 0.f;
    if constexpr (SOFTMAX)
        if (role_u && gr < nr) max_r = A.rmax[gr], inv_r = A.rinv[gr];
    auto load = [&](int64_t c0) {
        stage.load(c0);
        if constexpr (SOFTMAX)
            if (!role_u && tid < 2 * kIbTile) {
                const int64_t u = c0 + (tid & (kIbTile - 1));
                st_l = u < c_end ? (tid < kIbTile ? A.rmax[u] : A.rinv[u]) : 0.f;
            }
    };
    auto store = [&] {
        stage.store(tile);
        if constexpr (SOFTMAX)
            if (!role_u && tid < 2 * kIbTile) nrm_t[tid >> 6][tid & (kIbTile - 1)] = st_l;
    };

    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin + kIbTile - 1) / kIbTile) : 0;
    // the next tile in flight in registers while this one is multiplied (narrow D); at D > 64 the
    // registers go to the operands and the second block of the CU hides the load instead
    constexpr bool PREFETCH = DP <= 64;
    if (PREFETCH && ntiles > 0) load(c_begin);
    // tr-read lane roles: 16-lane group g, lane 4q + p of the group
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    for (int t = 0; t < ntiles; ++t) {
        const int64_t c0 = c_begin + (int64_t)t * kIbTile;
        if (!PREFETCH) load(c0);
        __syncthreads();  // every wave is done with the previous tile
        store();
        __syncthreads();
        if (PREFETCH && t + 1 < ntiles) load(c0 + kIbTile);  // in flight during this tile's MFMAs
        // the label Y = 1 sits at tile column diag of this lane's row: user u's own positive is
        // column row_base + u (user role), positive i's user is row i - row_base (item role)
        const int64_t dl = role_u ? A.row_base + gr - c0 : gr - A.row_base - c0;
        const int diag = (dl >= 0 && dl < kIbTile) ? (int)dl : -1;
        const int cols_here = (int)min((int64_t)kIbTile, c_end - c0);
        const bool row_ok = gr < nr;
        // wave-uniform: the whole 32 x 64 block is interior and label-free (most tiles)
        const bool fast = cols_here == kIbTile && __builtin_amdgcn_ballot_w64(diag >= 0 || !row_ok) == 0;
#pragma unroll
        for (int jc = 0; jc < 2; ++jc) {  // tile rows 32 jc .. 32 jc + 31
            f32x16 s2 = ibx_score<NP>(tile, jc, li, h, rf);
            // ---- dS^T in registers (lane: row u = r0 + li; register r: tile column c) -----------
            if constexpr (SOFTMAX) {
                // softmax: p = exp2(x z_scale - rmax) rinv (one fma, one hardware exp2, one multiply),
                // dS / inv_T = p - y; the interior fast path has no y and no range tests
                const float zc = A.z_scale;
#pragma unroll
                for (int q = 0; q < 4; ++q) {  // registers 4 q .. 4 q + 3: four consecutive tile columns
                    float4 m4, i4;
                    if (!role_u) {
                        const float* nt = nrm_t[0] + 32 * jc + 4 * h + 8 * q;
                        m4 = *reinterpret_cast<const float4*>(nt);
                        i4 = *reinterpret_cast<const float4*>(nt + kIbTile);
                    } else {
                        m4 = make_float4(max_r, max_r, max_r, max_r);
                        i4 = make_float4(inv_r, inv_r, inv_r, inv_r);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * q + e;
                        s2[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s2[r], zc, -f4at(m4, e))) * f4at(i4, e);
                    }
                }
                if (!fast) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lc = 32 * jc + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const bool ok = row_ok && lc < cols_here;
                        const float y = lc == diag ? 1.0f : 0.0f;
                        s2[r] = ok ? s2[r] - y : 0.f;
                    }
                }
            } else if (fast) {
                // every row and column in range, no label in this wave's block: y = 0 (the BCE terms
                // are the user role's)
                if (role_u) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float x = s2[r];
                        const float tx = ibx_exp_nabs(x);
                        const float sg = ibx_sigmoid(x, tx);
                        ibx_bce_free(x, tx, bce_lin, bce_log2);
                        s2[r] = sg * A.inv_T;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float x = s2[r];
                        s2[r] = ibx_sigmoid(x, ibx_exp_nabs(x)) * A.inv_T;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lc = 32 * jc + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool ok = row_ok && lc < cols_here;
                    const float y = lc == diag ? 1.0f : 0.0f;
                    const float x = s2[r];
                    const float tx = ibx_exp_nabs(x);
                    const float sg = ibx_sigmoid(x, tx);
                    if (role_u && ok) bce += ibx_bce_term(x, y, tx);
                    s2[r] = ok ? (sg - y) * A.inv_T : 0.f;
                }
            }
            // ---- product 2: acc[n] (rows u, columns 32 n ..) += dS . tile ---------------------------
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8_t a[3];
                {
                    const float4 x0 = make_float4(s2[8 * s + 0], s2[8 * s + 1], s2[8 * s + 2], s2[8 * s + 3]);
                    const float4 x1 = make_float4(s2[8 * s + 4], s2[8 * s + 5], s2[8 * s + 6], s2[8 * s + 7]);
                    uint2 pa[3], pb[3];
                    ibx_split(x0, pa);
                    ibx_split(x1, pb);
#pragma unroll
                    for (int q = 0; q < 3; ++q) a[q] = ibx_cat(pa[q], pb[q]);
                }
                // B: tile rows 32 jc + 16 s + 4 h + q (elements 0..3) and + 8 (elements 4..7)
                const int brow = 32 * jc + 16 * s + 4 * h + q4;
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    const int ch = 4 * n + 2 * (g & 1) + (p4 >> 1);
                    const int o0 = ibx_off(brow, ch) + 8 * (p4 & 1), o1 = ibx_off(brow + 8, ch) + 8 * (p4 & 1);
                    bf16x8_t b[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + q * kIbxPlane + o0));
                        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + q * kIbxPlane + o1));
                        const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        b[q] = __builtin_bit_cast(bf16x8_t, v);
                    }
                    acc[n] = ibx_mfma6<NP>(a, b, acc[n]);
                }
            }
        }
    }
    // ---- partial rows -> this split's slab ------------------------------------------------------
    float* slab = role_u ? A.slab_u + (int64_t)sp * A.B * D : A.slab_p + (int64_t)sp * A.Bc * D;
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t gr = r0 + lr;
            const int col = 32 * n + li;
            if (gr < nr && col < D) slab[gr * D + col] = SOFTMAX ? acc[n][r] * A.inv_T : acc[n][r];
        }
    if (!SOFTMAX && role_u) {
        bce = wave_sum(bce + (bce_lin + bce_log2 * 0.6931471805599453f));
        if (lane == 0) red[w] = bce;
        __syncthreads();
        if (tid == 0) {
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < NW; i += 2) sum += red[i] + red[i + 1];
            A.loss_part[blk] = sum;
        }
    }
}

// dU = sum of the user slabs, dP = sum of the item slabs, in split order.
__global__ void ib_reduce_kernel(InBatchArgs A) {
    const int64_t nu = A.B * A.D, total = nu + A.Bc * A.D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const bool u = i < nu;
        const int64_t e = u ? i : i - nu;
        const int64_t r = e / A.D;
        const int c = (int)(e - r * A.D);
        const float* slab = u ? A.slab_u : A.slab_p;
        const int64_t plane = (u ? A.B : A.Bc) * A.D;
        const int splits = u ? A.splits_u : A.splits_p;
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += slab[k * plane + e];
        if (u) A.dU[r * A.ld_du + c] = s;
        else A.dP[r * A.ld_dp + c] = s;
    }
}

// A loss sum over blocks' partial sums, in block order (fp64 accumulation): the one-op entries'
// loss (the fused step folds the parts into loss_finalize_kernel).
__global__ void ib_loss_sum_kernel(const float* __restrict__ parts, int n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += (double)parts[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- forward-only variant: the BCE sum of S, nothing else (validation in in-batch mode) ------------
// inbatch_x_kernel's user role cut down to product 1 and the BCE terms: a block owns 32 kIblWaves
// user rows and one split of the columns; a wave keeps its 32 rows' split-bf16 fragments in
// registers (ibx_row_frags), the positives stream through LDS in 64-row tiles of the same
// three-plane image (IbxStage) and each 32 x 32 score block is formed by the same five partial
// products (ibx_score).  Every in-range element then adds its BCE term with the training kernel's
// arithmetic (ibx_exp_nabs, ibx_bce_free on label-free interior blocks, ibx_bce_term elsewhere), so
// a batch's training and validation BCE are the same function of the same rows.  No dS, no second
// product, no transposed LDS reads, no slabs: a block writes one float.
// Without the dU accumulators and the second product's operands a wave needs fewer than 256
// registers at every D, so a block is 8 waves (two per SIMD: one wave's elementwise pass runs under
// the other's MFMAs), alone on its CU with the tile double buffered (96 KB LDS, one barrier per
// tile, the tile after next in flight in registers) and staged once for 256 rows.
constexpr int kIblWaves = 8;
constexpr int kIblRows = 32 * kIblWaves;
constexpr int kIblBlocks = 256;  // one resident round: a block per CU

//
// LOSS == TTAMM_INBATCH_SOFTMAX is the row log-sum-exp pass of the softmax loss over the same
// structure: instead of BCE terms a lane keeps, in log2 units (z = S * z_scale, z_scale =
// log2(e) / temperature), the running maximum m of its row's columns and the sum of exp2(z - m),
// rescaled when a tile raises m; only in-range elements enter (columns past c_end and rows past B
// are excluded, not added as zeros).  A row lives on lanes li and li + 32 (different columns): the
// halves are joined, then the block writes one (m, sum) pair per row into its split's plane of ms
// and, in the split whose columns hold it, the row's own positive's z into zpos.
// ib_lse_merge_kernel finishes the rows.
constexpr float kIbNegBig = -3.0e38f;  // "no column yet": finite, so m - m stays 0 and not NaN

template <int DP, int LOSS = TTAMM_INBATCH_BCE>
__global__ __launch_bounds__(64 * kIblWaves, 1) void inbatch_loss_kernel(InBatchLossArgs A) {
    constexpr bool SOFTMAX = LOSS == TTAMM_INBATCH_SOFTMAX;
    constexpr int NT = 64 * kIblWaves;
    constexpr int KS = DP / 16;            // k steps of the score product
    __shared__ __attribute__((aligned(16))) unsigned char tiles[2][3 * kIbxPlane];
    __shared__ float red[kIblWaves];

    const int blk = blockIdx.x;
    const int rb = blk / A.splits, sp = blk - rb * A.splits;
    const float* R = A.U;
    const float* C = A.P;
    const int64_t ldr = A.ldu, nr = A.B, ldc = A.ldp, nc = A.Bc;
    const int64_t c_begin = min(nc, (int64_t)sp * A.cols), c_end = min(nc, c_begin + A.cols);
    const int D = A.D;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)rb * kIblRows + 32 * w;

    bf16x8_t rf[KS][3];
    ibx_row_frags(R + (r0 + li) * ldr, r0 + li < nr, D, h, rf);
    float bce = 0.f, bce_lin = 0.f, bce_log2 = 0.f;
    float m_run = kIbNegBig, s_run = 0.f, z_pos = kIbNegBig;  // softmax: this lane's columns of its row

    IbxStage<DP, NT> stage{C, ldc, c_end, D, tid};
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin + kIbTile - 1) / kIbTile) : 0;
    if (ntiles > 0) {  // tile 0 in buffer 0, tile 1 in flight in registers
        stage.load(c_begin);
        stage.store(tiles[0]);
        if (ntiles > 1) stage.load(c_begin + kIbTile);
    }
    __syncthreads();
    const int64_t gr = r0 + li;
    const bool row_ok = gr < nr;
    for (int t = 0; t < ntiles; ++t) {
        const int64_t c0 = c_begin + (int64_t)t * kIbTile;
        const unsigned char* const tile = tiles[t & 1];
        // the label Y = 1 of this lane's user row sits at tile column diag
        const int64_t dl = A.row_base + gr - c0;
        const int diag = (dl >= 0 && dl < kIbTile) ? (int)dl : -1;
        const int cols_here = (int)min((int64_t)kIbTile, c_end - c0);
        // wave-uniform: the whole 32 x 64 block is interior and label-free (most tiles)
        const bool fast = cols_here == kIbTile && __builtin_amdgcn_ballot_w64(diag >= 0 || !row_ok) == 0;
#pragma unroll
        for (int jc = 0; jc < 2; ++jc) {  // tile rows 32 jc .. 32 jc + 31
            // lane = user row r0 + li, register r = tile column
            const f32x16 s2 = ibx_score<kIbxProducts<LOSS>>(tile, jc, li, h, rf);
            if constexpr (SOFTMAX) {
                // online log-sum-exp of these 16 columns: z_scale > 0, so max z = z_scale max x
                const float zc = A.z_scale;
                float mx = kIbNegBig;
                if (fast) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s2[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lc = 32 * jc + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (row_ok && lc < cols_here) mx = fmaxf(mx, s2[r]);
                        if (row_ok && lc == diag) z_pos = s2[r] * zc;
                    }
                }
                const float m_new = fmaxf(m_run, mx > kIbNegBig ? mx * zc : kIbNegBig);
                float add = 0.f;
                if (fast) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) add += __builtin_amdgcn_exp2f(__builtin_fmaf(s2[r], zc, -m_new));
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lc = 32 * jc + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s2[r], zc, -m_new));
                        add += (row_ok && lc < cols_here) ? e : 0.f;
                    }
                }
                s_run = s_run * __builtin_amdgcn_exp2f(m_run - m_new) + add;
                m_run = m_new;
            } else if (fast) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = s2[r];
                    ibx_bce_free(x, ibx_exp_nabs(x), bce_lin, bce_log2);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lc = 32 * jc + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool ok = row_ok && lc < cols_here;
                    const float y = lc == diag ? 1.0f : 0.0f;
                    const float x = s2[r];
                    const float tx = ibx_exp_nabs(x);
                    if (ok) bce += ibx_bce_term(x, y, tx);
                }
            }
        }
        // tile t + 1 (landed in registers during this tile's MFMAs) into the other buffer, last
        // read in tile t - 1 before that tile's barrier; tile t + 2 in flight
        if (t + 1 < ntiles) {
            stage.store(tiles[(t + 1) & 1]);
            if (t + 2 < ntiles) stage.load(c0 + 2 * kIbTile);
        }
        __syncthreads();
    }
    if constexpr (SOFTMAX) {
        // join the row's two half-wave lanes (h = 0 writes), then one pair per row and split
        const float m_o = __shfl_xor(m_run, 32, 64), s_o = __shfl_xor(s_run, 32, 64), z_o = __shfl_xor(z_pos, 32, 64);
        const float m = fmaxf(m_run, m_o);
        const float sum = s_run * __builtin_amdgcn_exp2f(m_run - m) + s_o * __builtin_amdgcn_exp2f(m_o - m);
        const float zp = fmaxf(z_pos, z_o);
        if (h == 0 && row_ok) {
            *reinterpret_cast<float2*>(A.ms + 2 * ((int64_t)sp * A.B + gr)) = make_float2(m, sum);
            const int64_t pc = A.row_base + gr;  // the row's own positive: in exactly one split
            if (pc >= c_begin && pc < c_end) A.zpos[gr] = zp;
        }
    } else {
        bce = wave_sum(bce + (bce_lin + bce_log2 * 0.6931471805599453f));
        if (lane == 0) red[w] = bce;
        __syncthreads();
        if (tid == 0) {
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < kIblWaves; i += 2) sum += red[i] + red[i + 1];
            A.loss_part[blk] = sum;
        }
    }
}

// The rows' splits merged in split order: lse[b] = m + log2(sum) (log2 units), term[b] =
// (lse[b] - zpos[b]) ln 2 = lse_b - S_bb / temperature, and the terms of a block's 256 rows summed
// by a fixed tree into loss_part[block].  No float atomics.  The gradient kernel gets the pair
// (rmax, rinv) = (m, 1 / sum) and not lse: p = exp2(z - m) / sum leaves a row of p summing to 1
// within the rounding of sum (about 6e-8), while one float lse of magnitude log2 Bc + max z carries
// half an ulp of its own (2e-7 to 5e-7) into every p of the row, and the sums over the batch that
// cancel under softmax (sum_j dP_j = sum_b (sum_j dS_bj) U_b) multiply exactly that.
__global__ __launch_bounds__(256) void ib_lse_merge_kernel(InBatchLossArgs A) {
    __shared__ float red[256];
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (b < A.B) {
        float2 v = *reinterpret_cast<const float2*>(A.ms + 2 * b);
        float m = v.x, sum = v.y;
        for (int k = 1; k < A.splits; ++k) {
            v = *reinterpret_cast<const float2*>(A.ms + 2 * ((int64_t)k * A.B + b));
            const float mn = fmaxf(m, v.x);
            sum = sum * exp2f(m - mn) + v.y * exp2f(v.x - mn);
            m = mn;
        }
        const float l = m + log2f(sum);
        term = (l - A.zpos[b]) * 0.6931471805599453f;
        A.lse[b] = l;
        A.term[b] = term;
        A.rmax[b] = m;
        A.rinv[b] = 1.0f / sum;  // the maximum's own term is 1: never a division by zero
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) A.loss_part[blockIdx.x] = red[0];
}

// ---- host: plans, the one problem check, the one D dispatch ------------------------------------------
// f(std::integral_constant<int, DP>) for the kernels' D class DP = D rounded up to 32, 64, 96 or 128
template <class F>
void ib_dispatch_dp(int D, F&& f) {
    switch ((D + 31) / 32 * 32) {
        case 32: f(std::integral_constant<int, 32>{}); break;
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 96: f(std::integral_constant<int, 96>{}); break;
        default: f(std::integral_constant<int, 128>{}); break;
    }
}

bool ib_exact_mfma() {  // TTAMM_FP32_MFMA=exact: the v_mfma_f32_32x32x2_f32 kernel (as gemm.hip's switch)
    const char* env = product_env("TTAMM_FP32_MFMA");
    return env && std::strcmp(env, "exact") == 0;
}

// The gradient kernels' blocks: row blocks of kIbRows x column splits of whole tiles per role.
void inbatch_plan(int64_t B, int64_t Bc, InBatchArgs& a) {
    a.rblk_u = (int)ceil_div(B, kIbRows);
    a.rblk_p = (int)ceil_div(Bc, kIbRows);
    // ~256 blocks per role (one resident round over both roles at two blocks per CU, each block
    // twice the columns of the former 512: C4 0.952 -> 0.924 ms/step, C2 in-batch 0.658 -> 0.625,
    // the C4 rank-of-8 shape unchanged, profiles/r04_s43_inbatch_blocks.txt); developer knob
    // TTAMM_IB_BLOCKS = blocks per role
    static const int64_t want_env = [] {
        const char* e = dev_env("TTAMM_IB_BLOCKS");
        return e ? (int64_t)std::atoi(e) : (int64_t)0;
    }();
    // (the all-gathered columns of a sharded step, Bc > 2B, keep 512: 3.63 vs 3.74 ms per step at
    // the emulated C4 rank of 8, profiles/r04_s43_inbatch_blocks.txt)
    const int64_t want = want_env > 0 ? want_env : (Bc > 2 * B ? 512 : 256);
    a.splits_u = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(Bc, kIbTile), ceil_div(want, a.rblk_u)));
    a.splits_p = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(B, kIbTile), ceil_div(want, a.rblk_p)));
    a.cols_u = ceil_div(ceil_div(Bc, a.splits_u), kIbTile) * kIbTile;
    a.cols_p = ceil_div(ceil_div(B, a.splits_p), kIbTile) * kIbTile;
    a.splits_u = (int)std::max<int64_t>(1, ceil_div(Bc, a.cols_u));
    a.splits_p = (int)std::max<int64_t>(1, ceil_div(B, a.cols_p));
}

// The forward-only kernel's blocks: row blocks of kIblRows users x column splits of whole 64-column
// tiles, ~kIblBlocks blocks: one 8-wave block per CU in a single resident round (the kernel's 96 KB
// of LDS and two waves per SIMD allow one).  A function of the shapes only: no environment
// variable moves the split.
void inbatch_loss_plan(int64_t B, int64_t Bc, InBatchLossArgs& a) {
    a.rblk = (int)ceil_div(B, kIblRows);
    const int64_t want = std::min<int64_t>(ceil_div(Bc, kIbTile), ceil_div(kIblBlocks, a.rblk));
    a.cols = ceil_div(ceil_div(Bc, std::max<int64_t>(1, want)), kIbTile) * kIbTile;
    a.splits = (int)std::max<int64_t>(1, ceil_div(Bc, a.cols));
}

// What every kernel here needs of its rows; labels_inside: each user's own positive is a column
// (the forward-only passes, which exclude nothing and look the label's logit up).
int inbatch_problem_check(const InBatchProblem& p, bool labels_inside) {
    int rc;
    if ((rc = inbatch_loss_check(p.D))) return rc;
    TTAMM_REQUIRE(p.B > 0 && p.Bc > 0 && p.B < (int64_t(1) << 31) && p.Bc < (int64_t(1) << 31), "in-batch: bad batch");
    TTAMM_REQUIRE(p.ldu % 4 == 0 && p.ldp % 4 == 0 && ((uintptr_t)p.U | (uintptr_t)p.P) % 16 == 0,
                  "in-batch: rows must be 16-byte aligned");
    TTAMM_REQUIRE(!labels_inside || (p.row_base >= 0 && p.row_base + p.B <= p.Bc),
                  "in-batch: the users' labels must lie inside the columns");
    return TTAMM_OK;
}

// plan, one two-role launch of the gradient kernel (fp32 MFMA, or split-bf16 in its LOSS form), then
// dU / dP = the slabs summed in split order
int launch_inbatch_grad(InBatchArgs& a, int loss, bool exact, hipStream_t s) {
    inbatch_plan(a.B, a.Bc, a);
    const dim3 g((unsigned)(a.rblk_u * a.splits_u + a.rblk_p * a.splits_p)), t(2 * kIbRows);
    ib_dispatch_dp(a.D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        if (exact) hipLaunchKernelGGL(inbatch_kernel<DP>, g, t, 0, s, a);
        // D = 128 at two blocks per CU spills ~20 registers and still beats one block per CU
        // (C4: 0.41 vs 0.50 ms per launch)
        else if (loss == TTAMM_INBATCH_SOFTMAX) hipLaunchKernelGGL((inbatch_x_kernel<DP, TTAMM_INBATCH_SOFTMAX>), g, t, 0, s, a);
        else hipLaunchKernelGGL((inbatch_x_kernel<DP, TTAMM_INBATCH_BCE>), g, t, 0, s, a);
    });
    TTAMM_LAUNCH_CHECK();
    const int64_t total = (a.B + a.Bc) * a.D;
    hipLaunchKernelGGL(ib_reduce_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 8192)), dim3(256), 0, s,
                       a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

// check, plan, one launch of the forward-only kernel in its LOSS form
int launch_inbatch_scores(InBatchLossArgs& a, int loss, hipStream_t s) {
    int rc;
    if ((rc = inbatch_problem_check(a, true))) return rc;
    inbatch_loss_plan(a.B, a.Bc, a);
    const dim3 g((unsigned)(a.rblk * a.splits)), t(64 * kIblWaves);
    ib_dispatch_dp(a.D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        if (loss == TTAMM_INBATCH_SOFTMAX) hipLaunchKernelGGL((inbatch_loss_kernel<DP, TTAMM_INBATCH_SOFTMAX>), g, t, 0, s, a);
        else hipLaunchKernelGGL((inbatch_loss_kernel<DP, TTAMM_INBATCH_BCE>), g, t, 0, s, a);
    });
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

}  // namespace

size_t inbatch_workspace_floats(int64_t B, int64_t Bc, int D, size_t* slab_u, size_t* slab_p, size_t* parts) {
    InBatchArgs a{};
    inbatch_plan(B, Bc, a);
    *slab_u = (size_t)a.splits_u * B * D;
    *slab_p = (size_t)a.splits_p * Bc * D;
    *parts = (size_t)a.rblk_u * a.splits_u;
    return *slab_u + *slab_p + *parts;
}

int inbatch_loss_check(int D) {
    TTAMM_REQUIRE(D > 0 && D % 4 == 0 && D <= 128, "in-batch negatives: embedding dim must be a multiple of 4, <= 128");
    return TTAMM_OK;
}

int inbatch_softmax_check(float inv_temperature) {
    TTAMM_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0.f,
                  "in-batch softmax: the inverse temperature must be finite and greater than zero");
    return TTAMM_OK;
}

int launch_inbatch(InBatchArgs& a, hipStream_t s) {
    int rc;
    if ((rc = inbatch_problem_check(a, false))) return rc;
    return launch_inbatch_grad(a, TTAMM_INBATCH_BCE, ib_exact_mfma(), s);
}

// ---- forward-only BCE sum (inbatch_loss_kernel) ----------------------------------------------------
int inbatch_loss_blocks(int64_t B, int64_t Bc) {
    InBatchLossArgs a{};
    inbatch_loss_plan(B, Bc, a);
    return a.rblk * a.splits;
}

int launch_inbatch_loss(InBatchLossArgs& a, hipStream_t s) { return launch_inbatch_scores(a, TTAMM_INBATCH_BCE, s); }

// ---- in-batch softmax: the LSE pass, then inbatch_x_kernel's softmax instantiation -----------------
// The LSE pass runs on inbatch_loss_plan's blocks (a function of the shapes only); its workspace is
// [ms: splits x B pairs | zpos B | lse B | term B | rmax B | rinv B | loss_part: one float per 256 rows].
int inbatch_lse_parts(int64_t B) { return (int)ceil_div(B, 256); }

size_t inbatch_lse_floats(int64_t B, int64_t Bc) {
    InBatchLossArgs a{};
    inbatch_loss_plan(B, Bc, a);
    return 2 * (size_t)a.splits * B + 5 * (size_t)B + (size_t)inbatch_lse_parts(B);
}

void inbatch_lse_bind(InBatchLossArgs& a, float* w) {
    inbatch_loss_plan(a.B, a.Bc, a);
    a.ms = w;  // even offsets: the pairs are read and written as float2
    a.zpos = a.ms + 2 * (size_t)a.splits * a.B;
    a.lse = a.zpos + a.B;
    a.term = a.lse + a.B;
    a.rmax = a.term + a.B;
    a.rinv = a.rmax + a.B;
    a.loss_part = a.rinv + a.B;
}

int launch_inbatch_lse(InBatchLossArgs& a, float inv_temperature, hipStream_t s) {
    int rc;
    if ((rc = inbatch_softmax_check(inv_temperature))) return rc;
    TTAMM_REQUIRE(a.ms && a.zpos && a.lse && a.term && a.rmax && a.rinv && a.loss_part && (uintptr_t)a.ms % 8 == 0,
                  "in-batch softmax: LSE workspace not bound");
    a.z_scale = inv_temperature * 1.4426950408889634f;
    if ((rc = launch_inbatch_scores(a, TTAMM_INBATCH_SOFTMAX, s))) return rc;
    hipLaunchKernelGGL(ib_lse_merge_kernel, dim3((unsigned)inbatch_lse_parts(a.B)), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_inbatch_softmax(InBatchArgs& a, InBatchLossArgs& l, float inv_temperature, hipStream_t s) {
    int rc;
    if ((rc = inbatch_problem_check(a, false))) return rc;
    if ((rc = launch_inbatch_lse(l, inv_temperature, s))) return rc;
    a.rmax = l.rmax, a.rinv = l.rinv;
    a.z_scale = l.z_scale;
    a.inv_T *= inv_temperature;  // dS = (p - y) inv_count / temperature
    return launch_inbatch_grad(a, TTAMM_INBATCH_SOFTMAX, false, s);
}

// ---- the four one-call ops (ttamm_inbatch_bce, _bce_loss, _softmax, _softmax_loss) -------------------
// An op's workspace: [the LSE block (softmax) | slab_u | slab_p | loss_part (with gradients)], or the
// forward-only BCE kernel's block sums alone.
size_t inbatch_op_workspace_bytes(int loss, bool grads, int64_t B, int64_t Bc, int D) {
    size_t su, sp, parts;
    const size_t lse = loss == TTAMM_INBATCH_SOFTMAX ? inbatch_lse_floats(B, Bc) : 0;
    if (grads) return sizeof(float) * (lse + inbatch_workspace_floats(B, Bc, D, &su, &sp, &parts));
    return sizeof(float) * (lse ? lse : (size_t)inbatch_loss_blocks(B, Bc));
}

int inbatch_op(int loss, bool grads, const InBatchProblem& p, float inv_count, float inv_temperature, float* dU,
               int64_t ld_du, float* dP, int64_t ld_dp, double* loss_sum, void* ws, size_t ws_bytes, hipStream_t s) {
    const bool softmax = loss == TTAMM_INBATCH_SOFTMAX;
    const std::string op = std::string(softmax ? "inbatch_softmax" : "inbatch_bce") + (grads ? "" : "_loss");
    int rc;
    TTAMM_REQUIRE(p.U && p.P && loss_sum && ws && (!grads || (dU && dP)), op + ": null argument");
    TTAMM_REQUIRE(p.B > 0 && p.Bc > 0 && p.D > 0 && p.ldu >= p.D && p.ldp >= p.D &&
                      (!grads || (ld_du >= p.D && ld_dp >= p.D)),
                  op + ": bad shape");
    TTAMM_REQUIRE(p.row_base >= 0 && p.row_base + p.B <= p.Bc,
                  op + ": row_base must place the B users' labels inside the Bc columns (0 <= row_base, "
                       "row_base + B <= Bc)");
    if (softmax && (rc = inbatch_softmax_check(inv_temperature))) return rc;
    if ((rc = inbatch_loss_check(p.D))) return rc;
    TTAMM_REQUIRE(ws_bytes >= inbatch_op_workspace_bytes(loss, grads, p.B, p.Bc, p.D), op + ": workspace too small");
    // bind: the forward pass's block, then the gradient pass's slabs
    float* w = static_cast<float*>(ws);
    InBatchLossArgs l{};
    static_cast<InBatchProblem&>(l) = p;
    if (softmax) {
        inbatch_lse_bind(l, w);
        w += inbatch_lse_floats(p.B, p.Bc);
    } else {
        l.loss_part = w;
    }
    InBatchArgs a{};
    static_cast<InBatchProblem&>(a) = p;
    if (grads) {
        size_t su, sp, parts;
        inbatch_workspace_floats(p.B, p.Bc, p.D, &su, &sp, &parts);
        a.slab_u = w, a.slab_p = w + su, a.loss_part = w + su + sp;
        a.inv_T = inv_count;
        a.dU = dU, a.ld_du = ld_du, a.dP = dP, a.ld_dp = ld_dp;
    }
    // run: the loss's partial sums are the LSE merge's (softmax), the gradient kernel's user blocks'
    // or the forward-only kernel's blocks'
    const float* parts = l.loss_part;
    int n = inbatch_lse_parts(p.B);
    if (softmax) {
        rc = grads ? launch_inbatch_softmax(a, l, inv_temperature, s) : launch_inbatch_lse(l, inv_temperature, s);
    } else if (grads) {
        rc = launch_inbatch(a, s);
        parts = a.loss_part, n = a.rblk_u * a.splits_u;
    } else {
        rc = launch_inbatch_loss(l, s);
        n = l.rblk * l.splits;
    }
    if (rc != TTAMM_OK) return rc;
    hipLaunchKernelGGL(ib_loss_sum_kernel, dim3(1), dim3(256), 0, s, parts, n, loss_sum);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

}  // namespace ttamm
