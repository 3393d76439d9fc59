// Optimizer side of the training step: the fused SparseAdam / AdamW / SGD updates of the touched
// table rows, the dense sweep, dense AdamW with the weight-gradient tail, and gradient clipping.
// The grouping of a batch's rows is group.hip, the deferred replay replay.hip, the per-element
// arithmetic optim_math.h.
//
// Row tables receive per-row gradient contributions from the batch (duplicates allowed).
// They are grouped by row (launch_coalesce, group.hip), so duplicate rows are summed in batch
// order — the order torch's CPU index_add / coalesce use (training.py:822 backward;
// _functional.py:44 grad.coalesce()).
//
// Tables in the dense group (the adaptive-mimic tables, adaptive_mimic.py:35-36, put in the
// AdamW group by training.py:306-307) are updated over EVERY row every step.  That sweep is
// split into (1) an AdamW update of the touched rows with their gradient into a side buffer,
// (2) a pure streaming AdamW(g = 0) pass over the whole table — the dominant HBM kernel of
// the step, 24 bytes per element — and (3) a scatter of the side rows over the swept table.
// The result equals one dense AdamW step over the full dense gradient.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cmath>
#include <cstring>

#include "kernels.h"

#pragma clang fp contract(off)  // (before optim_math.h: its functions are compiled under it)

#include "optim_math.h"

namespace ttamm {

namespace {

// Segmented sum of the row-gradient contributions, in two fixed-order levels so a hot row
// (a popular item with hundreds of duplicates in the batch) does not serialise one wave:
//   piece_sum: one wave per chunk of kPiece sorted positions sums each run of equal keys
//              inside its chunk ("piece") and stores it at the run's first position;
//   row_update: one wave per unique row adds its pieces in position order, then applies
//              the optimizer.  Both orders are fixed, so results are deterministic.
constexpr int kPiece = kCoalescePiece;
constexpr int kRowWaves = 4;

__device__ __forceinline__ const float* dA_row(const RowUpdateArgs& A, int64_t r) {
    // the fields as values first: a select between the two pointer FIELDS of the by-value kernel
    // argument compiled to a select of their addresses, copying the argument to scratch (24 B per
    // lane in row_update_kernel)
    const float* const lo = A.dA_lo;
    const float* const hi = A.dA_hi;
    const int64_t ld = A.ld_dA;
    if (const int64_t* xu = A.xu) {
        const int64_t u = xu[r];
        return u >= 0 ? lo + u * ld : hi + (~u) * ld;
    }
    return (r < A.split_row ? lo : hi) + r * ld;
}

// SDA: each position's dA row resolved once into LDS (compact exchange unit maps: their dependent
// load, and gradient rows past the buffer loads' 32-bit offsets); otherwise per column from its row
template <bool SDA>
__global__ __launch_bounds__(64 * kRowWaves) void piece_sum_kernel(RowUpdateArgs A) {
    __shared__ int64_t srows[kRowWaves][kPiece];
    __shared__ const float* sda[kRowWaves][kPiece];  // each position's dA row (resolved once: GateTower::xu)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t chunk = (int64_t)blockIdx.x * kRowWaves + w;
    const int64_t k0 = chunk * kPiece;
    if (k0 >= A.n) return;
    const int cnt = (int)min((int64_t)kPiece, A.n - k0);
    // only segments longer than a piece are summed in two levels (row_update sums the rest)
    if (__ballot(lane < cnt && A.seglong[k0 + lane] != 0) == 0ull) return;
    // positions of the chunk: lane p holds row / key / "last of a run" for position k0 + p
    int64_t my_row = 0;
    int my_key = 0, my_last = 1;
    if (lane < cnt) {
        my_row = A.rows[k0 + lane];
        my_key = A.keys[k0 + lane];
    }
    const int next_key = __shfl_down(my_key, 1, 64);
    if (lane + 1 < cnt) my_last = next_key != my_key;
    const uint64_t last_mask = __ballot(lane < cnt && my_last);
    const bool mimic = A.mimic.weight != nullptr;
    if (lane < kPiece) {  // read back uniformly inside the d loop
        srows[w][lane] = my_row;
        if (SDA) sda[w][lane] = mimic && lane < cnt ? dA_row(A, my_row) : nullptr;
    }
    __builtin_amdgcn_wave_barrier();
    const int D = A.dim;
    const bool idt = A.id.weight != nullptr;  // (a mimic-only pass leaves the ID table out)
    // SDA = false (no unit maps, launch_row_update): buffer loads, the position's row offset in the
    // scalar offset (the row is wave-uniform) and the column in one shared voffset — 64-bit
    // addresses per load had held the kernel at 288 registers, one wave per SIMD
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rE, rAlo, rAhi;
    if constexpr (!SDA) {
        rE = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.dE), 0, 0x7fffffff, 0x00020000);
        rAlo = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.dA_lo), 0, 0x7fffffff, 0x00020000);
        rAhi = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.dA_hi), 0, 0x7fffffff, 0x00020000);
    }
    for (int d = lane; d < D; d += 64) {
        float ve[kPiece], va[kPiece];
#pragma unroll
        for (int p = 0; p < kPiece; ++p) {  // issue every load of the chunk before adding
            if constexpr (SDA) {
                const int64_t r = srows[w][p];
                ve[p] = (idt && p < cnt) ? A.dE[r * A.ld_dE + d] : 0.f;
                va[p] = (mimic && p < cnt) ? sda[w][p][d] : 0.f;
            } else {
                const int r = __builtin_amdgcn_readfirstlane((int)srows[w][p]);
                ve[p] = (idt && p < cnt)
                    ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rE, 4 * d, (int)(4 * r * A.ld_dE), 0))
                    : 0.f;
                va[p] = (mimic && p < cnt)
                    ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r < A.split_row ? rAlo : rAhi, 4 * d,
                                                                                     (int)(4 * r * A.ld_dA), 0))
                    : 0.f;
            }
        }
        float ge = 0.f, ga = 0.f;
        int start = 0;
#pragma unroll
        for (int p = 0; p < kPiece; ++p) {
            if (p < cnt) {
                ge += ve[p];
                ga += va[p];
                if ((last_mask >> p) & 1ull) {
                    if (idt) A.piece_e[(k0 + start) * D + d] = ge;
                    if (mimic) A.piece_a[(k0 + start) * D + d] = ga;
                    ge = ga = 0.f;
                    start = p + 1;
                }
            }
        }
    }
}

// float4 views of table / gradient rows (dim % 4 == 0, 16-byte aligned rows: checked by the
// launcher)
__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 addf4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One unique row per `lanes_per_row` lanes (the power of two >= dim / 4, at most 64: set by the
// launcher), one float4 column per lane and trip of the column loop; a trip's table loads are
// issued before its gradient sums.  (Several columns per lane with every load up front ran the C2
// item launch 70 -> 91 us at 183 registers: DESIGN §11.)
__global__ __launch_bounds__(64 * kRowWaves) void row_update_kernel(RowUpdateArgs A) {
    const int lane = threadIdx.x & 63;
    const int lpr = A.lanes_per_row, rpw = 64 / lpr;
    const int64_t u = ((int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6)) * rpw + lane / lpr;
    const int sub = lane % lpr;
    if (u >= A.n || u >= (int64_t)A.n_unique[0] || step_poisoned(A.status)) return;
    const int64_t k0 = A.seg_start[u], k1 = A.seg_start[u + 1];
    const int64_t key = A.keys[k0];
    const int D = A.dim;
    const bool mimic = A.mimic.weight != nullptr;
    const bool idt = A.id.weight != nullptr;  // (a mimic-only pass leaves the ID table out)
    const bool direct = k1 - k0 <= kPiece;
    // nn.Embedding padding_idx: no gradient into that row (SparseAdam: not in the sparse gradient at
    // all, so the row is left as it is; AdamW: a zero gradient row)
    const bool pad_row = idt && A.id.has_padding_idx && key == A.id.padding_idx;
    auto each = [](float4& p, float4& m, float4& v, float4 g, auto&& f) {
        f(p.x, m.x, v.x, g.x);
        f(p.y, m.y, v.y, g.y);
        f(p.z, m.z, v.z, g.z);
        f(p.w, m.w, v.w, g.w);
    };
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int d = 4 * sub; d < D; d += 4 * lpr) {
        const int64_t o = key * D + d;
        // the table rows first: they do not depend on the gradient sums below
        float4 ip = idt ? ldf4(A.id.weight + o) : z4;
        float4 im = idt ? ldf4(A.id.exp_avg + o) : z4;
        float4 iv = idt ? ldf4(A.id.exp_avg_sq + o) : z4;
        float4 mp = mimic ? ldf4(A.mimic.weight + o) : z4;
        float4 mm = mimic ? ldf4(A.mimic.exp_avg + o) : z4;
        float4 mv = mimic ? ldf4(A.mimic.exp_avg_sq + o) : z4;
        float4 ge, ga;
        if (direct) {  // the row's contributions in batch order
            const int64_t r0 = A.rows[k0];
            const float* e0 = A.dE + r0 * A.ld_dE;
            const float* a0 = mimic ? dA_row(A, r0) : nullptr;
            ge = idt ? ldf4(e0 + d) : z4;
            ga = mimic ? ldf4(a0 + d) : z4;
            for (int64_t k = k0 + 1; k < k1; ++k) {
                const int64_t r = A.rows[k];
                const float* er = A.dE + r * A.ld_dE;
                const float* ar = mimic ? dA_row(A, r) : nullptr;
                if (idt) ge = addf4(ge, ldf4(er + d));
                if (mimic) ga = addf4(ga, ldf4(ar + d));
            }
        } else {  // pieces (piece_sum_kernel), then the pieces in order
            ge = idt ? ldf4(A.piece_e + k0 * D + d) : z4;
            ga = mimic ? ldf4(A.piece_a + k0 * D + d) : z4;
            for (int64_t k = (k0 / kPiece + 1) * kPiece; k < k1; k += kPiece) {
                if (idt) ge = addf4(ge, ldf4(A.piece_e + k * D + d));
                if (mimic) ga = addf4(ga, ldf4(A.piece_a + k * D + d));
            }
        }
        if (A.grad_scale) {  // clip_grad_norm_: g *= coef (training.py:824-825)
            const float c = *A.grad_scale;
            ge = make_float4(ge.x * c, ge.y * c, ge.z * c, ge.w * c);
            ga = make_float4(ga.x * c, ga.y * c, ga.z * c, ga.w * c);
        }
        if (pad_row) ge = z4;
        if (!idt) {
            // mimic-only pass
        } else if (A.id.optimizer == TTAMM_OPT_SPARSE_ADAM) {
            if (!pad_row)
                each(ip, im, iv, ge, [&](float& p, float& m, float& v, float g) { sparse_adam_elem(p, m, v, g, A.sp); });
        } else {
            each(ip, im, iv, ge, [&](float& p, float& m, float& v, float g) { adam_elem(p, m, v, g, A.ad); });
        }
        if (!idt || (A.id.optimizer == TTAMM_OPT_SPARSE_ADAM && pad_row)) {
            // untouched
        } else if (A.id.optimizer == TTAMM_OPT_SPARSE_ADAM || A.id.last_step) {
            // SparseAdam, or deferred mode: the row was caught up before the forward
            stf4(A.id.weight + o, ip);
            stf4(A.id.exp_avg + o, im);
            stf4(A.id.exp_avg_sq + o, iv);
        } else {
            float* sd = A.side_id + u * 3 * D;
            stf4(sd + d, ip);
            stf4(sd + D + d, im);
            stf4(sd + 2 * D + d, iv);
        }
        if (mimic) {
            each(mp, mm, mv, ga, [&](float& p, float& m, float& v, float g) { adam_elem(p, m, v, g, A.ad); });
            if (A.mimic.last_step) {
                stf4(A.mimic.weight + o, mp);
                stf4(A.mimic.exp_avg + o, mm);
                stf4(A.mimic.exp_avg_sq + o, mv);
            } else {
                float* sd = A.side_mimic + u * 3 * D;
                stf4(sd + d, mp);
                stf4(sd + D + d, mm);
                stf4(sd + 2 * D + d, mv);
            }
        }
    }
    if (sub == 0) {
        if (idt && A.id.optimizer != TTAMM_OPT_SPARSE_ADAM && A.id.last_step) {
            A.id.last_step[key] = A.dense_step;
            if (A.id.touched && !pad_row) A.id.touched[key] = 1;
        }
        if (mimic && A.mimic.last_step) {
            A.mimic.last_step[key] = A.dense_step;
            if (A.mimic.touched) A.mimic.touched[key] = 1;
        }
    }
}

// Streaming AdamW(g = 0) over whole tables: 12 B read + 12 B written per element.
__global__ __launch_bounds__(256) void dense_sweep_kernel(SweepArgs A) {
    if (step_poisoned(A.status)) return;
    for (int s = 0; s < A.count; ++s) {
        const SweepSeg& S = A.seg[s];
        const int64_t n4 = S.n >> 2;
        float4* P = reinterpret_cast<float4*>(S.p);
        float4* Mm = reinterpret_cast<float4*>(S.m);
        float4* V = reinterpret_cast<float4*>(S.v);
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            float4 p = P[i], m = Mm[i], v = V[i];
            adam_elem_g0(p.x, m.x, v.x, A.ad);
            adam_elem_g0(p.y, m.y, v.y, A.ad);
            adam_elem_g0(p.z, m.z, v.z, A.ad);
            adam_elem_g0(p.w, m.w, v.w, A.ad);
            P[i] = p;
            Mm[i] = m;
            V[i] = v;
        }
        // scalar tail
        for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S.n; i += stride) {
            float p = S.p[i], m = S.m[i], v = S.v[i];
            adam_elem_g0(p, m, v, A.ad);
            S.p[i] = p;
            S.m[i] = m;
            S.v[i] = v;
        }
    }
}

__global__ void side_scatter_kernel(const int32_t* __restrict__ n_unique, const int32_t* __restrict__ keys,
                                    const int32_t* __restrict__ seg_start, const float* __restrict__ side, int64_t n,
                                    int dim, ttamm_table t, const uint32_t* __restrict__ status) {
    if (step_poisoned(status)) return;
    const int64_t total = n * dim;
    const int64_t nu = n_unique[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = i / dim;
        if (u >= nu) return;
        const int d = (int)(i - u * dim);
        const int64_t key = keys[seg_start[u]];
        const float* sd = side + u * 3 * dim;
        const int64_t o = key * dim + d;
        t.weight[o] = sd[d];
        t.exp_avg[o] = sd[dim + d];
        t.exp_avg_sq[o] = sd[2 * dim + d];
    }
}

__global__ void dense_adam_kernel(DenseAdamArgs A, int64_t total) {
    if (step_poisoned(A.status)) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int64_t off = i;
        int t = 0;
        while (t < A.count - 1 && off >= A.t[t].n) {
            off -= A.t[t].n;
            ++t;
        }
        const DenseTensor& T = A.t[t];
        float p = T.p[off], m = T.m[off], v = T.v[off];
        adam_elem(p, m, v, A.grad_scale ? T.g[off] * *A.grad_scale : T.g[off], A.ad);
        T.p[off] = p;
        T.m[off] = m;
        T.v[off] = v;
    }
}

// The one-process step's tail: wgrad_reduce_kernel and dense_adam_kernel in one pass.  A block
// owns a 32 (n_in, the bias row n_in == N included) x 32 (m_out) tile of one problem.  Phase 1, a
// thread per 4 consecutive m_out of a slab row: s = 0; s += slab[0]; s += slab[1]; ... per
// element, the loads of kTailDepth splits issued before their adds (the slabs are [n_in][m_out],
// so a wave reads whole 128-B segments).  The sums cross LDS, and phase 2 runs with n_in fastest:
// the gradient store and the parameter's p / m / v traffic ([m_out][n_in]) are contiguous, and
// adam_elem sees the operands dense_adam_kernel gives it.
constexpr int kTailTile = 32, kTailDepth = 16;
struct WgradTailArgs {
    WgradBatch wb;
    WgradTail tail;
};
static_assert(sizeof(WgradTailArgs) <= 4096, "one kernel argument");

__global__ __launch_bounds__(256) void wgrad_tail_kernel(WgradTailArgs A) {
    const KArg(WgradTailArgs)* ka = (const KArg(WgradTailArgs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    __shared__ float sums[kTailTile][kTailTile + 1];
    int tile = blockIdx.x, pi = 0;
    for (; pi < ka->wb.count - 1; ++pi) {
        const int nt = ((ka->wb.p[pi].N + kTailTile) / kTailTile) * ((ka->wb.p[pi].M + kTailTile - 1) / kTailTile);
        if (tile < nt) break;
        tile -= nt;
    }
    const KArg(WgradProblem)& P = ka->wb.p[pi];
    const KArg(WgradTailParam)& Q = ka->tail.t[pi];
    const int Mo = P.M, Nn = P.N, splits = P.splits;
    const int tiles_m = (Mo + kTailTile - 1) / kTailTile;
    const int n0 = (tile / tiles_m) * kTailTile, m0 = (tile % tiles_m) * kTailTile;
    const int64_t plane = (int64_t)(Nn + 1) * Mo;
    const int tid = threadIdx.x;
    {
        const int nr = tid >> 3, mc = (tid & 7) * 4;
        const int n = n0 + nr, m = m0 + mc;
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};  // (native vectors: the chunk stays in registers)
        if (n <= Nn && m < Mo) {
            const float* src = P.slab + (int64_t)n * Mo + m;
            if ((Mo & 3) == 0 && (reinterpret_cast<uintptr_t>(P.slab) & 15) == 0) {  // m + 3 < Mo
                int sp = 0;
                for (; sp + kTailDepth <= splits; sp += kTailDepth) {
                    f32x4_t v[kTailDepth];
#pragma unroll
                    for (int i = 0; i < kTailDepth; ++i)
                        v[i] = *reinterpret_cast<const f32x4_t*>(src + (int64_t)(sp + i) * plane);
                    // (the scheduler otherwise sinks each load to its add to save registers)
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < kTailDepth; ++i) s += v[i];
                }
                if (sp < splits) {  // the last partial chunk: loads past the end re-read the last split
                    f32x4_t v[kTailDepth - 1];
#pragma unroll
                    for (int i = 0; i < kTailDepth - 1; ++i)
                        v[i] = *reinterpret_cast<const f32x4_t*>(src + (int64_t)min(sp + i, splits - 1) * plane);
#pragma unroll
                    for (int i = 0; i < kTailDepth - 1; ++i) {
                        const f32x4_t t = s + v[i];
                        s = sp + i < splits ? t : s;
                    }
                }
            } else {  // rows that are not 16-byte aligned: element by element
                for (int sp = 0; sp < splits; ++sp) {
                    const float* q = src + (int64_t)sp * plane;
                    s.x += q[0];
                    if (m + 1 < Mo) s.y += q[1];
                    if (m + 2 < Mo) s.z += q[2];
                    if (m + 3 < Mo) s.w += q[3];
                }
            }
        }
        sums[nr][mc] = s.x, sums[nr][mc + 1] = s.y, sums[nr][mc + 2] = s.z, sums[nr][mc + 3] = s.w;
    }
    __syncthreads();
    const bool poisoned = step_poisoned(A.tail.status);
    float* const gw = P.grad_w;
    float* const gb = P.grad_b;
    float* const pw = Q.pw;
    float* const mw = Q.mw;
    float* const vw = Q.vw;
    float* const pb = Q.pb;
    float* const mb = Q.mb;
    float* const vb = Q.vb;
#pragma unroll
    for (int j = 0; j < kTailTile * kTailTile / 256; ++j) {
        const int idx = j * 256 + tid;
        const int nn = idx & (kTailTile - 1), mm = idx / kTailTile;
        const int n = n0 + nn, m = m0 + mm;
        if (n > Nn || m >= Mo) continue;
        const float g = sums[nn][mm];
        const bool bias = n == Nn;
        const int64_t o = bias ? (int64_t)m : (int64_t)m * Nn + n;
        float* gp = bias ? gb : gw;
        float* pp = bias ? pb : pw;
        float* pm = bias ? mb : mw;
        float* pv = bias ? vb : vw;
        if (gp) gp[o] = g;
        if (poisoned || pp == nullptr) continue;
        float p = pp[o], mo = pm[o], v = pv[o];
        adam_elem(p, mo, v, g, A.tail.ad);
        pp[o] = p;
        pm[o] = mo;
        pv[o] = v;
    }
}

// ---- clip_grad_norm_ (training.py:824-825; torch/nn/utils/clip_grad.py) ---------------------
// sum over a tower table pair's touched rows of |sum of the row's gradient contributions|^2
// (the dense gradient tensor's rows; the padding row's ID gradient is zero), one thread per
// (row, 4 columns), the row's contributions summed in batch order
__global__ void rows_sumsq_kernel(RowUpdateArgs A, float* __restrict__ partials) {
    __shared__ float red[4];
    const int dim4 = A.dim >> 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t u = e / dim4;
    float acc = 0.f;
    if (u < A.n && u < (int64_t)A.n_unique[0]) {
        const int d = (int)(e - u * dim4) * 4;
        const int64_t k0 = A.seg_start[u], k1 = A.seg_start[u + 1];
        const int64_t key = A.keys[k0];
        const bool mimic = A.mimic.weight != nullptr;
        float4 ge = make_float4(0.f, 0.f, 0.f, 0.f), ga = ge;
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t r = A.rows[k];
            ge = addf4(ge, ldf4(A.dE + r * A.ld_dE + d));
            if (mimic) ga = addf4(ga, ldf4(dA_row(A, r) + d));
        }
        if (A.id.has_padding_idx && key == A.id.padding_idx) ge = make_float4(0.f, 0.f, 0.f, 0.f);
        acc = (ge.x * ge.x + ge.y * ge.y) + (ge.z * ge.z + ge.w * ge.w) +
              ((ga.x * ga.x + ga.y * ga.y) + (ga.z * ga.z + ga.w * ga.w));
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void dense_sumsq_kernel(DenseAdamArgs A, int64_t total, float* __restrict__ partials) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t off = i;
        int t = 0;
        while (t < A.count - 1 && off >= A.t[t].n) {
            off -= A.t[t].n;
            ++t;
        }
        const float g = A.t[t].g[off];
        acc += g * g;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one block: the partials summed in a fixed order (fp64), then torch's fp32 coefficient
// clip_coef = max_norm / (total_norm + 1e-6), clamped to <= 1
__global__ void clip_coef_kernel(const float* __restrict__ partials, int n, float max_norm, float* coef) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(red[0]);
        const float c = max_norm / (total + 1e-6f);
        *coef = c < 1.0f ? c : 1.0f;
    }
}


__global__ void sum_partials_kernel(const float* __restrict__ partials, int n, float* out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)red[0];
}

__global__ void sparse_adam_rows_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                        int dim, const int64_t* __restrict__ rows, const float* __restrict__ grad,
                                        int64_t n, SparseConsts c) {
    const int64_t total = n * dim;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = i / dim;
        const int d = (int)(i - u * dim);
        const int64_t o = rows[u] * dim + d;
        float p = w[o], mm = m[o], vv = v[o];
        sparse_adam_elem(p, mm, vv, grad[i], c);
        w[o] = p;
        m[o] = mm;
        v[o] = vv;
    }
}

}  // namespace

// RN(1/c) for a positive normal fp32 c: the double quotient rounded to fp32 may be off by one
// ulp (double rounding), so pick among it and its neighbours the one with the smallest
// |1 - y*c|, evaluated exactly in double (24-bit x 24-bit products fit in 53 bits).
float correctly_rounded_reciprocal(float c) {
    const float y0 = (float)(1.0 / (double)c);
    float best = y0;
    double err = std::fabs(1.0 - (double)y0 * (double)c);
    for (float y : {std::nextafter(y0, 0.f), std::nextafter(y0, INFINITY)}) {
        const double e = std::fabs(1.0 - (double)y * (double)c);
        if (e < err) {
            err = e;
            best = y;
        }
    }
    return best;
}

AdamConsts make_adam_consts(double lr, double beta1, double beta2, double eps, double wd, int decoupled,
                            int64_t step) {
    AdamConsts c;
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    c.decay = (float)(1.0 - lr * wd);
    c.w1 = (float)(1.0 - beta1);
    c.b2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.neg_step = (float)(-(lr / bc1));
    c.bc2_sqrt = (float)std::pow(bc2, 0.5);
    c.inv_bc2_sqrt = correctly_rounded_reciprocal(c.bc2_sqrt);
    const double ns = -(lr / bc1);
    if (ns != 0.0) {
        c.fast_ibc = (float)(1.0 / (std::sqrt(bc2) * ns));
        c.fast_eps = (float)(eps / ns);
    } else {  // lr = 0: r = rcp(+inf) = +0, p = fma(m, 0, p) = p (torch: p + (-0) * (m / denom))
        c.fast_ibc = 0.f;
        c.fast_eps = INFINITY;
    }
    c.wd = (float)wd;
    c.decoupled = decoupled;
    c.fast_g0 = 0;
    c.sgd = 0, c.sgd_neg_lr = 0.f, c.sgd_mom = 0.f, c.sgd_damp1 = 0.f, c.sgd_first = 0, c.sgd_nesterov = 0;
    return c;
}

AdamConsts make_sgd_consts(double lr, double wd, double momentum, double dampening, int nesterov, int first) {
    AdamConsts c;
    std::memset(&c, 0, sizeof(c));
    c.sgd = 1;
    c.sgd_neg_lr = (float)(-lr);
    c.wd = (float)wd;
    c.sgd_mom = (float)momentum;
    c.sgd_damp1 = (float)(1.0 - dampening);
    c.sgd_first = first ? 1 : 0;
    c.sgd_nesterov = nesterov ? 1 : 0;
    return c;
}

SparseConsts make_sparse_consts(double lr, double beta1, double beta2, double eps, int64_t step) {
    SparseConsts c;
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    c.w1 = (float)(1.0 - beta1);
    c.w2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.neg_step = (float)(-(lr * std::sqrt(bc2) / bc1));
    return c;
}

int launch_row_update(const RowUpdateArgs& args, hipStream_t s) {
    if (args.n <= 0) return TTAMM_OK;
    RowUpdateArgs a = args;
    TTAMM_REQUIRE(a.dim % 4 == 0 && (!a.id.weight || a.ld_dE % 4 == 0) && (!a.mimic.weight || a.ld_dA % 4 == 0),
                  "row update: dim and gradient leading dims must be multiples of 4");
    a.lanes_per_row = 1;
    while (a.lanes_per_row < a.dim / 4 && a.lanes_per_row < 64) a.lanes_per_row *= 2;
    // per-column dA rows unless the unit maps are on (their dependent load): the LDS-resolved form
    // cost the one-process C2 step 7 us (0.6616 vs 0.6545 ms, profiles/r05_s42_piece_sum.txt)
    // (the buffer-load form takes 32-bit byte offsets of the gradient rows: positions index them)
    const bool small = 4 * a.n * std::max<int64_t>(a.ld_dE, a.ld_dA) < (int64_t(1) << 31);
    const bool sda = a.xu != nullptr || !small;
    if (sda) hipLaunchKernelGGL(piece_sum_kernel<true>, dim3((unsigned)ceil_div(ceil_div(a.n, kPiece), kRowWaves)),
                       dim3(64 * kRowWaves), 0, s, a);
    else hipLaunchKernelGGL(piece_sum_kernel<false>, dim3((unsigned)ceil_div(ceil_div(a.n, kPiece), kRowWaves)),
                       dim3(64 * kRowWaves), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    const int64_t rows_per_block = (int64_t)kRowWaves * (64 / a.lanes_per_row);
    hipLaunchKernelGGL(row_update_kernel, dim3((unsigned)ceil_div(a.n, rows_per_block)), dim3(64 * kRowWaves), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_dense_sweep(const SweepArgs& a, hipStream_t s) {
    int64_t total4 = 0;
    for (int i = 0; i < a.count; ++i) {
        TTAMM_REQUIRE(((uintptr_t)a.seg[i].p | (uintptr_t)a.seg[i].m | (uintptr_t)a.seg[i].v) % 16 == 0,
                      "dense sweep: tables must be 16-byte aligned");
        total4 += a.seg[i].n >> 2;
    }
    if (a.count == 0) return TTAMM_OK;
    // 2048 blocks x 256 threads: 8 blocks per CU, grid-stride over the tables
    hipLaunchKernelGGL(dense_sweep_kernel, dim3(grid_blocks(total4, 256, 2048)), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_side_scatter(const int32_t* n_unique, const int32_t* keys, const int32_t* seg_start, const float* side,
                        int64_t n, int dim, ttamm_table t, const uint32_t* status, hipStream_t s) {
    if (n <= 0) return TTAMM_OK;
    hipLaunchKernelGGL(side_scatter_kernel, dim3(grid_blocks(n * dim)), dim3(256), 0, s, n_unique, keys, seg_start, side,
                       n, dim, t, status);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int rows_sumsq_blocks(int64_t n, int dim) { return (int)std::max<int64_t>(1, ceil_div(n * (dim / 4), 256)); }

int launch_rows_sumsq(const RowUpdateArgs& a, float* partials, hipStream_t s) {
    if (a.n <= 0) return TTAMM_OK;
    TTAMM_REQUIRE(a.dim % 4 == 0, "clip: dim must be a multiple of 4");
    hipLaunchKernelGGL(rows_sumsq_kernel, dim3((unsigned)rows_sumsq_blocks(a.n, a.dim)), dim3(256), 0, s, a, partials);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_dense_sumsq(const DenseAdamArgs& a, float* partials, hipStream_t s) {
    int64_t total = 0;
    for (int i = 0; i < a.count; ++i) total += a.t[i].n;
    if (total == 0) {
        TTAMM_HIP(hipMemsetAsync(partials, 0, kDenseSumsqBlocks * sizeof(float), s));
        return TTAMM_OK;
    }
    hipLaunchKernelGGL(dense_sumsq_kernel, dim3(kDenseSumsqBlocks), dim3(256), 0, s, a, total, partials);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_clip_coef(const float* partials, int n, float max_norm, float* coef, hipStream_t s) {
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, s, partials, n, max_norm, coef);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_sum_partials(const float* partials, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, partials, n, out);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_dense_adam(const DenseAdamArgs& a, hipStream_t s) {
    int64_t total = 0;
    for (int i = 0; i < a.count; ++i) total += a.t[i].n;
    if (total == 0) return TTAMM_OK;
    hipLaunchKernelGGL(dense_adam_kernel, dim3(grid_blocks(total, 256, 4096)), dim3(256), 0, s, a, total);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_wgrad_tail(const WgradBatch& wb, const WgradTail& tail, hipStream_t s) {
    WgradTailArgs a;
    a.wb = wb;
    a.wb.tail = nullptr;
    a.tail = tail;
    int64_t tiles = 0;
    for (int i = 0; i < wb.count; ++i)
        tiles += ceil_div(wb.p[i].N + 1, kTailTile) * ceil_div(wb.p[i].M, kTailTile);
    if (tiles == 0) return TTAMM_OK;
    hipLaunchKernelGGL(wgrad_tail_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_sparse_adam_rows(float* w, float* m, float* v, int dim, const int64_t* rows, const float* grad, int64_t n,
                            SparseConsts c, hipStream_t s) {
    if (n <= 0) return TTAMM_OK;
    hipLaunchKernelGGL(sparse_adam_rows_kernel, dim3(grid_blocks(n * dim)), dim3(256), 0, s, w, m, v, dim, rows, grad,
                       n, c);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

}  // namespace ttamm
