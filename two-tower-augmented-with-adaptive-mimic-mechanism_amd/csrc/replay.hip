// Deferred exact AdamW / Adam / SGD with g = 0 for the dense-group tables (ttamm.h
// ttamm_table.last_step): instead of sweeping every row every step, each step's constants go into
// a history ring (step_begin_kernel) and a row that is `lag` steps behind replays them — over a
// rolling slice of each table, a flush, or the catch-up lists that group.hip builds for the rows
// a batch touches.  The operations per element are the eager sweep's (optim_math.h), so the bits
// agree.
#include <cstring>
#include <type_traits>

#include "kernels.h"

#pragma clang fp contract(off)  // (before optim_math.h: its functions are compiled under it)

#include "optim_math.h"

namespace ttamm {

namespace {

constexpr int kMaxHistory = kMaxAdamHistory;

__global__ void step_begin_kernel(const uint32_t* status, int64_t* applied, AdamConsts* hist, int cap, int64_t step,
                                  AdamConsts c) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || step_poisoned(status)) return;
    if (applied) applied[0] += 1;
    if (hist) hist[step % cap] = c;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The per-step constants a g = 0 replay reads (the AdamW fast path loads the first 24 B)
struct ReplayConsts {
    float decay, w1, b2, eps, neg_step, inv_bc2_sqrt, bc2_sqrt, wd, w2, fast_ibc, fast_eps, pad0;
};
// The fast decoupled replay's constants as element pairs (each value twice), read as whole 64-bit
// operands by the packed loop.  Built from one float, the compiler broadcast it into both halves
// of a v_pk_* with op_sel, and picked a destination pair whose low register was that broadcast
// source (v_pk_fma_f32 v[48:49], v[54:55], v[48:49], v[48:49] op_sel_hi:[1,0,1]); run beside the
// feature MLP's GEMMs on the main stream, that replay gave run-to-run different parameters
// (tools/diag/deferred_c2.py, profiles/r04_replay_pk_overlap.txt).  With pair operands the halves
// of every packed instruction read only their own lane.
struct ReplayPairs {
    f32x2 decay, w1, b2, ibc, eps;
    float pad0, pad1;
};
static_assert(sizeof(ReplayPairs) == sizeof(ReplayConsts), "one LDS ring size for both layouts");

__device__ __forceinline__ float lo_of(float x) { return x; }
__device__ __forceinline__ float lo_of(f32x2 x) { return x.x; }

// ---- the frame the replay kernels share ------------------------------------------------------
// Entry r of a segment: its row and the step l it is current to — from the catch-up list, or from
// the row range and last[row].  false: the row is current, nothing to replay.
__device__ __forceinline__ bool replay_row(const KArg(ReplaySeg)& S, bool by_list, int32_t target, uint32_t r,
                                           int64_t& row, int32_t& l) {
    if (by_list) {
        row = S.list_rows[r];
        l = target - S.list_lag[r];
    } else {
        row = S.row_lo + r;
        l = S.last[row];
        if (l >= target) return false;
    }
    return true;
}
// (The V-float4 loads and stores of p / m / v stay typed out in each kernel: as helpers taking the
// register arrays by reference they moved the register allocation of every instantiation, e.g.
// replay_kernel<false, false, 2> 47 -> 57 VGPRs: profiles/optim_refactor_codegen.txt.)

// a staged ring entry as the constants adam_elem_t reads
__device__ __forceinline__ AdamConsts consts_of(const ReplayConsts& h) {
    AdamConsts c;
    c.decay = h.decay, c.w1 = h.w1, c.b2 = h.b2, c.eps = h.eps, c.neg_step = h.neg_step;
    c.bc2_sqrt = h.bc2_sqrt, c.inv_bc2_sqrt = h.inv_bc2_sqrt, c.wd = h.wd, c.w2 = h.w2;
    c.fast_ibc = h.fast_ibc, c.fast_eps = h.fast_eps;
    return c;
}

// One thread per V float4s of a row (dim % (4 V) == 0: 4 V independent dependency chains per
// thread sharing each step's constants, at float4 columns q and q + dim / (4 V)); blockIdx.y =
// segment.  A row current to step l is brought to A.target by replaying adam_elem(g = 0) with
// the constants of steps l+1 .. target — the operations the eager sweep applies, so the bits
// agree.  Rows come from a range (the rolling slice, the flush: untouched rows of one slice share
// their lag) or from a catch-up list sorted by lag (launch_prepare_segs), so the lanes of a wave
// run one trip count.
template <bool DECOUPLED, bool FAST, int V>
__global__ __launch_bounds__(256) void replay_kernel(ReplayArgs) {
    constexpr bool PKL = DECOUPLED && FAST;  // the packed-pair loop
    using HC = typename std::conditional<PKL, ReplayPairs, ReplayConsts>::type;
    const KArg(ReplayArgs)* ka = (const KArg(ReplayArgs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(ReplaySeg)& S = ka->seg[blockIdx.y];
    if (step_poisoned(ka->status)) return;
    // the history ring unrolled twice in LDS (2 cap entries, sized at launch: ~6 KB by default),
    // so a row's steps l+1 .. target are consecutive entries from (l + 1) % cap — no wrap test
    // and no address arithmetic beyond a pointer increment in the VALU-bound loop
    extern __shared__ __attribute__((aligned(16))) unsigned char replay_lds[];
    HC* H2 = reinterpret_cast<HC*>(replay_lds);
    const int cap = ka->cap;
    for (int i = threadIdx.x; i < 2 * cap; i += blockDim.x) {
        const AdamConsts& h = ka->hist[i < cap ? i : i - cap];
        if constexpr (PKL)
            H2[i] = ReplayPairs{f32x2{h.decay, h.decay}, f32x2{h.w1, h.w1}, f32x2{h.b2, h.b2},
                                f32x2{h.fast_ibc, h.fast_ibc}, f32x2{h.fast_eps, h.fast_eps}, 0.f, 0.f};
        else
            H2[i] = ReplayConsts{h.decay, h.w1, h.b2, h.eps, h.neg_step, h.inv_bc2_sqrt, h.bc2_sqrt, h.wd, h.w2,
                                 h.fast_ibc, h.fast_eps, 0.f};
    }
    __syncthreads();
    const int dim = S.dim;
    const uint32_t per_row = (uint32_t)(dim >> 2) / V;  // threads per row
    const int32_t target = ka->target;
    const bool by_list = S.list_rows != nullptr;
    const uint32_t nrows = by_list ? (uint32_t)S.list_cnt[0] : (uint32_t)(S.row_hi - S.row_lo);
    const uint32_t total = nrows * per_row;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / per_row, q = e - r * per_row;
        int64_t row;
        int32_t l;
        if (!replay_row(S, by_list, target, r, row, l)) continue;
        const int64_t o = row * dim + 4 * (int64_t)q;
        const HC* hc = H2 + (l + 1) % cap;
        const HC* const hend = hc + (target - l);
        if (DECOUPLED && S.touched && S.touched[row] == 0) {
            // a row never given a gradient: m = v = +0.0 stay so, and each step is p *= decay
            // (the cold path below, bit for bit) — only the parameter row moves
            float4 p[V];
#pragma unroll
            for (int i = 0; i < V; ++i) p[i] = *reinterpret_cast<const float4*>(S.p + o + (int64_t)(4 * per_row) * i);
            for (; hc != hend; ++hc) {
                const float decay = lo_of(hc->decay);
#pragma unroll
                for (int i = 0; i < V; ++i)
                    p[i].x = p[i].x * decay, p[i].y = p[i].y * decay, p[i].z = p[i].z * decay, p[i].w = p[i].w * decay;
            }
#pragma unroll
            for (int i = 0; i < V; ++i) *reinterpret_cast<float4*>(S.p + o + (int64_t)(4 * per_row) * i) = p[i];
            continue;
        }
        float4 p[V], m[V], v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int64_t oi = o + (int64_t)(4 * per_row) * i;
            p[i] = *reinterpret_cast<const float4*>(S.p + oi);
            m[i] = *reinterpret_cast<const float4*>(S.m + oi);
            v[i] = *reinterpret_cast<const float4*>(S.v + oi);
        }
        // A cold row (first moment +0.0: never given a gradient) stays cold under g = 0 (m = fma(w1,
        // -0, 0) = +0), and its update term neg_step * (0 * r) is -0.0, which leaves p * decay
        // unchanged for every p — so its replay is p *= decay, v *= b2 per step, bit for bit what
        // the full update computes, without the two transcendentals.  Most rows of a large table
        // are cold for many steps (C4: the in-batch positives touch ~8 K of 6.25 M rows a step).
        uint32_t mbits = 0u, vbits = 0u;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            mbits |= __float_as_uint(m[i].x) | __float_as_uint(m[i].y) | __float_as_uint(m[i].z) | __float_as_uint(m[i].w);
            vbits |= __float_as_uint(v[i].x) | __float_as_uint(v[i].y) | __float_as_uint(v[i].z) | __float_as_uint(v[i].w);
        }
        // a cold row's m is unchanged (+0.0), and a virgin row's v too (+0.0 * b2 = +0.0): their
        // stores are skipped (the flush after a short run is mostly such rows: 24 -> 16 B per element)
        const bool keep_m = DECOUPLED && mbits == 0u, keep_v = keep_m && vbits == 0u;
        if (DECOUPLED && mbits == 0u) {
            for (; hc != hend; ++hc) {
                const float decay = lo_of(hc->decay), b2 = lo_of(hc->b2);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    p[i].x = p[i].x * decay, p[i].y = p[i].y * decay, p[i].z = p[i].z * decay, p[i].w = p[i].w * decay;
                    v[i].x = v[i].x * b2, v[i].y = v[i].y * b2, v[i].z = v[i].z * b2, v[i].w = v[i].w * b2;
                }
            }
        }
        if constexpr (PKL) {
            // adam_elem_t<true, true, true> on element pairs, written with 2-wide vectors so every
            // multiply / fma issues as one v_pk_* for two elements (the denominator's fma included):
            // the same IEEE operations per element, so the dense sweep's scalar form gives the same bits
            for (; hc != hend; ++hc) {
                const f32x2 decay = hc->decay, w1 = hc->w1, b2 = hc->b2, ibc = hc->ibc, eps = hc->eps;
#pragma unroll
                for (int i = 0; i < V; ++i) {
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        f32x2 P = half ? f32x2{p[i].z, p[i].w} : f32x2{p[i].x, p[i].y};
                        f32x2 M = half ? f32x2{m[i].z, m[i].w} : f32x2{m[i].x, m[i].y};
                        f32x2 Q = half ? f32x2{v[i].z, v[i].w} : f32x2{v[i].x, v[i].y};
                        P = P * decay;
                        M = __builtin_elementwise_fma(w1, -M, M);
                        Q = Q * b2;
                        const f32x2 Sq = {__builtin_amdgcn_sqrtf(Q.x), __builtin_amdgcn_sqrtf(Q.y)};
                        const f32x2 Dn = __builtin_elementwise_fma(Sq, ibc, eps);
                        const f32x2 R = {__builtin_amdgcn_rcpf(Dn.x), __builtin_amdgcn_rcpf(Dn.y)};
                        P = __builtin_elementwise_fma(M, R, P);
                        if (half) {
                            p[i].z = P.x, p[i].w = P.y, m[i].z = M.x, m[i].w = M.y, v[i].z = Q.x, v[i].w = Q.y;
                        } else {
                            p[i].x = P.x, p[i].y = P.y, m[i].x = M.x, m[i].y = M.y, v[i].x = Q.x, v[i].y = Q.y;
                        }
                    }
                }
            }
        } else {
            for (; hc != hend; ++hc) {
                const AdamConsts c = consts_of(*hc);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    adam_elem_t<DECOUPLED, true, FAST>(p[i].x, m[i].x, v[i].x, 0.f, c);
                    adam_elem_t<DECOUPLED, true, FAST>(p[i].y, m[i].y, v[i].y, 0.f, c);
                    adam_elem_t<DECOUPLED, true, FAST>(p[i].z, m[i].z, v[i].z, 0.f, c);
                    adam_elem_t<DECOUPLED, true, FAST>(p[i].w, m[i].w, v[i].w, 0.f, c);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int64_t oi = o + (int64_t)(4 * per_row) * i;
            *reinterpret_cast<float4*>(S.p + oi) = p[i];
            if (!keep_m) *reinterpret_cast<float4*>(S.m + oi) = m[i];
            if (!keep_v) *reinterpret_cast<float4*>(S.v + oi) = v[i];
        }
    }
}

// The deferred SGD(g = 0) replay (torch.optim.SGD in the dense group, training.py:1324-1330): an
// untouched row's step is p' = p + lr-scaled momentum of its own decay term,
//     g = p wd;  buf = fma(g, 1 - dampening, buf momentum) (buf = g on a first step);
//     p = fma(nesterov ? fma(buf, momentum, g) : buf, -lr, p)
// — linear in (p, buf), no transcendentals.  Each replayed step applies sgd_elem(g = 0) with that
// step's constants from the history ring (AdamConsts: sgd_neg_lr, sgd_mom, sgd_damp1, sgd_first,
// sgd_nesterov, wd), exactly the operations the eager sweep applies, so deferred == eager bit for
// bit.  momentum == 0: m and v alias the parameter (no state), the stores write p three times.
// Constants are read per lane from the ring in global memory (L1/L2-resident, a few dozen bytes a
// step); the loop is a handful of FMAs per element-step, so it is HBM-bound like the row traffic.
template <int V>
__global__ __launch_bounds__(256) void replay_sgd_kernel(ReplayArgs) {
    const KArg(ReplayArgs)* ka = (const KArg(ReplayArgs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(ReplaySeg)& S = ka->seg[blockIdx.y];
    if (step_poisoned(ka->status)) return;
    const AdamConsts* hist = ka->hist;
    const int cap = ka->cap;
    const int dim = S.dim;
    const uint32_t per_row = (uint32_t)(dim >> 2) / V;
    const int32_t target = ka->target;
    const bool by_list = S.list_rows != nullptr;
    const uint32_t nrows = by_list ? (uint32_t)S.list_cnt[0] : (uint32_t)(S.row_hi - S.row_lo);
    const uint32_t total = nrows * per_row;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / per_row, q = e - r * per_row;
        int64_t row;
        int32_t l;
        if (!replay_row(S, by_list, target, r, row, l)) continue;
        const int64_t o = row * dim + 4 * (int64_t)q;
        float4 p[V], m[V], v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int64_t oi = o + (int64_t)(4 * per_row) * i;
            p[i] = *reinterpret_cast<const float4*>(S.p + oi);
            m[i] = *reinterpret_cast<const float4*>(S.m + oi);
            v[i] = *reinterpret_cast<const float4*>(S.v + oi);
        }
        int j = (l + 1) % cap;
        for (int32_t k = l; k < target; ++k) {
            AdamConsts c = hist[j];
            c.sgd = 1;
            j = j + 1 == cap ? 0 : j + 1;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                sgd_elem(p[i].x, m[i].x, v[i].x, 0.f, c);
                sgd_elem(p[i].y, m[i].y, v[i].y, 0.f, c);
                sgd_elem(p[i].z, m[i].z, v[i].z, 0.f, c);
                sgd_elem(p[i].w, m[i].w, v[i].w, 0.f, c);
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int64_t oi = o + (int64_t)(4 * per_row) * i;
            *reinterpret_cast<float4*>(S.p + oi) = p[i];
            *reinterpret_cast<float4*>(S.m + oi) = m[i];
            *reinterpret_cast<float4*>(S.v + oi) = v[i];
        }
    }
}

// row ranges only: last[row] = target (stamp 1) or max(last[row], target) (stamp 2) after the
// replay (list segments were stamped by their build)
__global__ void stamp_kernel(ReplayArgs) {
    const KArg(ReplayArgs)* ka = (const KArg(ReplayArgs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(ReplaySeg)& S = ka->seg[blockIdx.y];
    if (step_poisoned(ka->status) || S.list_rows != nullptr) return;
    const bool at_least = ka->stamp == 2;
    for (int64_t r = S.row_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < S.row_hi;
         r += (int64_t)gridDim.x * blockDim.x) {
        if (at_least) atomicMax(&S.last[r], ka->target);
        else S.last[r] = ka->target;
    }
}

}  // namespace

int launch_step_begin(const uint32_t* status, int64_t* applied, AdamConsts* hist, int cap, int64_t step,
                      const AdamConsts& c, hipStream_t s) {
    TTAMM_REQUIRE(!hist || (cap > 1 && cap <= kMaxHistory), "adam history: capacity must be in [2, 512]");
    if (!hist && !applied) return TTAMM_OK;
    hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(64), 0, s, status, applied, hist, hist ? cap : 2, step, c);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

template <int V>
static void launch_replay_v(const ReplayArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    // lds: the history ring staged per block (replay_kernel)
    if (a.sgd) {
        hipLaunchKernelGGL((replay_sgd_kernel<V>), grid, dim3(256), 0, s, a);
        return;
    }
    if (a.fast_g0) {
        if (a.decoupled) hipLaunchKernelGGL((replay_kernel<true, true, V>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((replay_kernel<false, true, V>), grid, dim3(256), lds, s, a);
    } else if (a.decoupled) {
        hipLaunchKernelGGL((replay_kernel<true, false, V>), grid, dim3(256), lds, s, a);
    } else {
        hipLaunchKernelGGL((replay_kernel<false, false, V>), grid, dim3(256), lds, s, a);
    }
}

int launch_replay(const ReplayArgs& a, hipStream_t s, void* const* ev) {
    if (a.count == 0) return TTAMM_OK;
    TTAMM_REQUIRE(a.count <= kMaxReplaySegs && a.hist && a.cap > 1 && a.cap <= kMaxHistory,
                  "replay: bad arguments");
    int64_t most = 0;
    bool v2 = true;  // two float4s per thread when every segment's dim is a multiple of 8
    for (int i = 0; i < a.count; ++i) v2 = v2 && a.seg[i].dim % 8 == 0;
    const int V = v2 ? 2 : 1;
    for (int i = 0; i < a.count; ++i) {
        const ReplaySeg& g = a.seg[i];
        TTAMM_REQUIRE(g.p && g.m && g.v && (g.last || g.list_rows), "replay: table without deferred state");
        TTAMM_REQUIRE(!g.list_rows || (g.list_lag && g.list_cnt), "replay: catch-up list incomplete");
        TTAMM_REQUIRE(g.dim % 4 == 0 && ((uintptr_t)g.p | (uintptr_t)g.m | (uintptr_t)g.v) % 16 == 0,
                      "replay: tables must be 16-byte aligned with dim % 4 == 0");
        const int64_t n = g.row_hi - g.row_lo;  // lists: the batch positions bound the listed rows
        TTAMM_REQUIRE(n >= 0 && n * (g.dim / 4) < (int64_t(1) << 31), "replay: more than 2^31 float4s in a segment");
        most = n * (g.dim / 4 / V) > most ? n * (g.dim / 4 / V) : most;
    }
    if (most == 0) return TTAMM_OK;
    const dim3 grid(grid_blocks(most, 256, 16384), a.count);
    const size_t lds = (size_t)2 * a.cap * sizeof(ReplayConsts);
    if (ev && ev[0]) TTAMM_HIP(hipEventRecord((hipEvent_t)ev[0], s));
    if (v2) launch_replay_v<2>(a, grid, lds, s);
    else launch_replay_v<1>(a, grid, lds, s);
    TTAMM_LAUNCH_CHECK();
    if (ev && ev[1]) TTAMM_HIP(hipEventRecord((hipEvent_t)ev[1], s));
    if (a.stamp) {
        int64_t rows = 0;
        for (int i = 0; i < a.count; ++i) rows = a.seg[i].row_hi - a.seg[i].row_lo > rows ? a.seg[i].row_hi - a.seg[i].row_lo : rows;
        hipLaunchKernelGGL(stamp_kernel, dim3(grid_blocks(rows, 256, 4096), a.count), dim3(256), 0, s, a);
        TTAMM_LAUNCH_CHECK();
    }
    return TTAMM_OK;
}

}  // namespace ttamm
