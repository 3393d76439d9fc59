// Grouping of a batch's row ids for the table updates, and the catch-up lists of the deferred
// replay.
//
// Row tables receive per-row gradient contributions from the batch (duplicates allowed).  They
// are grouped by row (launch_coalesce: counts and first occurrences through per-row scratch, a
// one-block scan, a scatter, then each row's positions put back in ascending order), so duplicate
// rows are summed in batch order — the order torch's CPU index_add / coalesce use (training.py:822
// backward; _functional.py:44 grad.coalesce()).  The count pass also serves the deferred replay
// (replay.hip): the rows a batch touches that are behind are listed by lag (launch_prepare_segs).
#include <algorithm>
#include <climits>
#include <cstring>

#include "kernels.h"

#pragma clang fp contract(off)

namespace ttamm {

namespace {

constexpr int kMaxHistory = kMaxAdamHistory;

// ---- grouping of a batch's row ids (launch_coalesce) ----------------------------------------
// Each row's count and first position, for up to two towers (blockIdx.y = tower).  first[key]
// holds INT_MAX - (first position): 0 = untouched, and atomicMax keeps the earliest.  Each tower's
// first block also zeroes its catch-up list counters (CatchupList cnt + fill), which the next
// launch reads
__global__ void co_count_seg_kernel(PrepSegs) {
    const KArg(PrepSegs)* ka = (const KArg(PrepSegs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(PrepSeg)& S = ka->seg[blockIdx.y];
    if (blockIdx.x == 0 && S.list_cnt)
        for (int i = threadIdx.x; i < 2 * (ka->cap + 1); i += blockDim.x) S.list_cnt[i] = 0;  // cnt, fill
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S.n) return;
    const int64_t key = S.idx[p];
    atomicAdd(&S.cnt[key], 1);
    atomicMax(&S.first[key], (int32_t)(INT_MAX - p));
}

// Entry i of the segment scan: (flag, count) — a position's leader flag and its row's count,
// or (sorted mode, entries = the key range) whether key i occurs and its count.
__device__ __forceinline__ void co_entry(int by_key, int64_t i, const int64_t* __restrict__ idx,
                                         const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                         int32_t& f, int32_t& c) {
    if (by_key) {
        c = cnt[i];
        f = c > 0;
    } else {
        const int64_t key = idx[i];
        f = first[key] == (int32_t)(INT_MAX - i);
        c = f ? cnt[key] : 0;
    }
}

// block-wide inclusive scan of (f, c) over 256 threads
__device__ __forceinline__ void block_scan2(int32_t& f, int32_t& c, int32_t* sf, int32_t* sc) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t a = __shfl_up(f, o, 64), b = __shfl_up(c, o, 64);
        if (lane >= o) {
            f += a;
            c += b;
        }
    }
    if (lane == 63) {
        sf[w] = f;
        sc[w] = c;
    }
    __syncthreads();
    int32_t pf = 0, pc = 0;
    for (int i = 0; i < w; ++i) {
        pf += sf[i];
        pc += sc[i];
    }
    f += pf;
    c += pc;
}

// pass 1 of the segment scan: each 256-entry tile's totals
__global__ __launch_bounds__(256) void co_tile_sum_kernel(int64_t n, int by_key, const int64_t* __restrict__ idx,
                                                          const int32_t* __restrict__ cnt,
                                                          const int32_t* __restrict__ first,
                                                          int32_t* __restrict__ tile_f, int32_t* __restrict__ tile_c) {
    __shared__ int32_t sf[4], sc[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t f = 0, c = 0;
    if (i < n) co_entry(by_key, i, idx, cnt, first, f, c);
    block_scan2(f, c, sf, sc);
    if (threadIdx.x == 255) {
        tile_f[blockIdx.x] = f;
        tile_c[blockIdx.x] = c;
    }
}

// pass 2: exclusive scan of the tile totals (one block; tiles are few), n_unique, total
__global__ __launch_bounds__(1024) void co_tile_scan_kernel(int64_t tiles, int32_t* __restrict__ tile_f,
                                                            int32_t* __restrict__ tile_c, int32_t* __restrict__ seg_start,
                                                            int32_t* __restrict__ n_unique) {
    __shared__ int32_t sf[1024], sc[1024];
    const int t = threadIdx.x;
    const int64_t chunk = (tiles + 1023) / 1024;
    const int64_t lo = min(tiles, t * chunk), hi = min(tiles, lo + chunk);
    int32_t f_sum = 0, c_sum = 0;
    for (int64_t i = lo; i < hi; ++i) {
        f_sum += tile_f[i];
        c_sum += tile_c[i];
    }
    sf[t] = f_sum;
    sc[t] = c_sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int32_t a = t >= o ? sf[t - o] : 0, b = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sf[t] += a;
        sc[t] += b;
        __syncthreads();
    }
    int32_t rf = sf[t] - f_sum, rc = sc[t] - c_sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t a = tile_f[i], b = tile_c[i];
        tile_f[i] = rf;
        tile_c[i] = rc;
        rf += a;
        rc += b;
    }
    if (t == 1023) {
        n_unique[0] = sf[t];
        seg_start[sf[t]] = sc[t];
    }
}

// pass 3: every flagged entry's segment index and start; the index goes to lead[position]
// (first-occurrence order) or first[key] (sorted mode)
__global__ __launch_bounds__(256) void co_tile_write_kernel(int64_t n, int by_key, const int64_t* __restrict__ idx,
                                                            const int32_t* __restrict__ cnt, int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ tile_f,
                                                            const int32_t* __restrict__ tile_c,
                                                            int32_t* __restrict__ lead, int32_t* __restrict__ seg_start) {
    __shared__ int32_t sf[4], sc[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t f = 0, c = 0;
    if (i < n) co_entry(by_key, i, idx, cnt, first, f, c);
    int32_t fi = f, ci = c;
    block_scan2(fi, ci, sf, sc);
    if (f) {
        const int32_t u = tile_f[blockIdx.x] + fi - 1;
        seg_start[u] = tile_c[blockIdx.x] + ci - c;
        if (by_key) first[i] = u;
        else lead[i] = u;
    }
}

// every position into its row's segment (order within a segment: arbitrary, fixed next)
__global__ void co_fill_kernel(const int64_t* __restrict__ idx, int64_t n, int by_key,
                               const int32_t* __restrict__ lead, const int32_t* __restrict__ first,
                               int32_t* __restrict__ fill, const int32_t* __restrict__ seg_start,
                               int32_t* __restrict__ vals_tmp, int32_t* __restrict__ keys_out,
                               int32_t* __restrict__ n_big) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) n_big[0] = 0;  // the long-segment list of the ordering pass
    if (p >= n) return;
    const int64_t key = idx[p];
    const int32_t u = by_key ? first[key] : lead[INT_MAX - first[key]];  // the leader's segment
    const int32_t slot = seg_start[u] + atomicAdd(&fill[key], 1);
    vals_tmp[slot] = (int32_t)p;
    keys_out[slot] = (int32_t)key;
}

// Segment ordering: every segment's positions in ascending order (so duplicate rows sum in
// batch order), the long-segment flags, and the row's scratch back to zero.  One thread per
// segment sorts up to kOrderSmall positions in registers (nearly every row of a batch occurs
// once or a few times); longer segments (hot rows) are listed in `big` and ranked by whole
// blocks (co_order_big_kernel).
constexpr int kOrderSmall = 16;

__device__ __forceinline__ void co_reset(const CoalesceWs& W, int32_t key) {
    W.cnt[key] = 0;
    W.first[key] = 0;
    W.fill[key] = 0;
}

__global__ __launch_bounds__(256) void co_order_small_kernel(CoalesceWs W, int32_t* __restrict__ big,
                                                             int32_t* __restrict__ n_big) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= W.n_unique[0]) return;
    const int32_t k0 = W.seg_start[u], L = W.seg_start[u + 1] - k0;
    if (L > kOrderSmall) {
        big[atomicAdd(n_big, 1)] = (int32_t)u;
        return;
    }
    int32_t v[kOrderSmall];
#pragma unroll
    for (int i = 0; i < kOrderSmall; ++i) v[i] = i < L ? W.vals_tmp[k0 + i] : INT_MAX;
#pragma unroll
    for (int i = 1; i < kOrderSmall; ++i)  // insertion sort, fully unrolled (registers only)
#pragma unroll
        for (int j = i; j > 0; --j) {
            const int32_t a = v[j - 1], b = v[j];
            v[j - 1] = min(a, b);
            v[j] = max(a, b);
        }
    const int32_t longseg = L > kCoalescePiece ? 1 : 0;
#pragma unroll
    for (int i = 0; i < kOrderSmall; ++i)
        if (i < L) {
            W.vals_out[k0 + i] = v[i];
            W.seglong[k0 + i] = longseg;
        }
    co_reset(W, W.keys_out[k0]);
}

// Long segments: the positions are distinct integers, so each one's rank within the segment is
// the number of the segment's positions below it — a bitmap over the segment's position range in
// LDS, per-word prefix popcounts, one lookup per position: O(range / 32 + L) per segment (a
// Zipf-hot item of a C2 batch spans ~50K positions: 1.5K words).  A range wider than the bitmap
// falls back to counting ranks (L^2 / threads).
constexpr int kBitWords = 6144;  // position range up to 196,608 (48 KB of LDS with the prefixes)
__global__ __launch_bounds__(256) void co_order_big_kernel(CoalesceWs W, const int32_t* __restrict__ big,
                                                           const int32_t* __restrict__ n_big) {
    __shared__ uint32_t bits[kBitWords];
    __shared__ int32_t pre[kBitWords];
    __shared__ int32_t sf[4], sc[4], smin[4], smax[4];
    const int nb = n_big[0];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const int32_t u = big[b];
        const int32_t k0 = W.seg_start[u], k1 = W.seg_start[u + 1], L = k1 - k0;
        const int32_t longseg = L > kCoalescePiece ? 1 : 0;
        // the segment's position range
        int32_t lo = INT_MAX, hi = -1;
        for (int32_t j = threadIdx.x; j < L; j += blockDim.x) {
            const int32_t v = W.vals_tmp[k0 + j];
            lo = min(lo, v);
            hi = max(hi, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        __syncthreads();  // the previous segment's LDS reads are done
        if (lane == 0) {
            smin[wv] = lo;
            smax[wv] = hi;
        }
        __syncthreads();
        lo = min(min(smin[0], smin[1]), min(smin[2], smin[3]));
        hi = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        const int32_t nw = ((hi - lo) >> 5) + 1;
        if (nw <= kBitWords) {
            for (int32_t w = threadIdx.x; w < nw; w += blockDim.x) bits[w] = 0u;
            __syncthreads();
            for (int32_t j = threadIdx.x; j < L; j += blockDim.x) {
                const int32_t d = W.vals_tmp[k0 + j] - lo;
                atomicOr(&bits[d >> 5], 1u << (d & 31));
            }
            __syncthreads();
            // exclusive prefix of the words' popcounts: contiguous chunks per thread, block scan
            const int32_t chunk = (nw + (int32_t)blockDim.x - 1) / (int32_t)blockDim.x;
            const int32_t w0 = min(nw, (int32_t)threadIdx.x * chunk), w1 = min(nw, w0 + chunk);
            int32_t c = 0;
            for (int32_t w = w0; w < w1; ++w) c += __popc(bits[w]);
            int32_t f = 0, ci = c;
            block_scan2(f, ci, sf, sc);
            int32_t run = ci - c;
            for (int32_t w = w0; w < w1; ++w) {
                pre[w] = run;
                run += __popc(bits[w]);
            }
            __syncthreads();
            for (int32_t j = threadIdx.x; j < L; j += blockDim.x) {
                const int32_t v = W.vals_tmp[k0 + j];
                const int32_t d = v - lo;
                const int32_t r = pre[d >> 5] + __popc(bits[d >> 5] & ((1u << (d & 31)) - 1u));
                W.vals_out[k0 + r] = v;
            }
        } else {
            for (int32_t j = threadIdx.x; j < L; j += blockDim.x) {
                const int32_t v = W.vals_tmp[k0 + j];
                int32_t rank = 0;
                for (int32_t i = k0; i < k1; ++i) rank += W.vals_tmp[i] < v ? 1 : 0;
                W.vals_out[k0 + rank] = v;
            }
        }
        for (int32_t j = threadIdx.x; j < L; j += blockDim.x) W.seglong[k0 + j] = longseg;
        if (threadIdx.x == 0) co_reset(W, W.keys_out[k0]);
    }
}

// ---- catch-up lists (launch_prepare_segs) ----------------------------------------------------
// lag of batch position p, or 0 when p is not its row's first occurrence or the row is current
__device__ __forceinline__ int32_t catchup_lag(const int64_t* __restrict__ idx, int64_t p, int64_t n,
                                               const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                               int32_t target, int64_t& row) {
    if (p >= n) return 0;
    row = idx[p];
    if (first[row] != (int32_t)(INT_MAX - p)) return 0;
    const int32_t lag = target - last[row];
    return lag > 0 ? lag : 0;
}

// rows per lag: a block histogram in LDS, then one atomic per (block, lag); cnt[0] = all rows
__device__ __forceinline__ void catchup_count_block(const int64_t* __restrict__ idx, int64_t n,
                                                    const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                    int32_t target, int cap, int32_t* __restrict__ cnt, int32_t* h) {
    for (int i = threadIdx.x; i <= cap; i += blockDim.x) h[i] = 0;
    __syncthreads();
    int64_t row = 0;
    const int32_t lag = catchup_lag(idx, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n, first, last, target, row);
    if (lag > 0) {
        atomicAdd(&h[lag], 1);
        atomicAdd(&h[0], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= cap; i += blockDim.x)
        if (h[i]) atomicAdd(&cnt[i], h[i]);
}

// both towers' lists in one launch (blockIdx.y = tower)
__global__ __launch_bounds__(256) void catchup_count_seg_kernel(PrepSegs) {
    const KArg(PrepSegs)* ka = (const KArg(PrepSegs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(PrepSeg)& S = ka->seg[blockIdx.y];
    __shared__ int32_t h[kMaxHistory + 1];
    if (step_poisoned(ka->status) || S.list_cnt == nullptr) return;
    catchup_count_block(S.idx, S.n, S.first, S.last[0], ka->target, ka->cap, S.list_cnt, h);
}

// each listed row into its lag's range of the list (longest lag first: lag b starts at
// sum_{b' > b} cnt[b']), in block order within a lag (atomics: any order — every row's replay is
// independent of the others), then stamped current in every table of the tower
__device__ __forceinline__ void catchup_scatter_block(const int64_t* __restrict__ idx, int64_t n,
                                                      const int32_t* __restrict__ first, int32_t* const* last,
                                                      int nlast, int32_t target, int cap,
                                                      const int32_t* __restrict__ cnt, int32_t* __restrict__ fill,
                                                      int32_t* __restrict__ rows, int32_t* __restrict__ lags,
                                                      int32_t (*suf)[kMaxHistory + 2], int32_t* h, int32_t* base) {
    const int tid = threadIdx.x;
    for (int i = tid; i <= cap + 1; i += blockDim.x) {
        suf[0][i] = (i >= 1 && i <= cap) ? cnt[i] : 0;
        if (i <= cap) h[i] = 0;
    }
    __syncthreads();
    int cur = 0;
    for (int off = 1; off <= cap; off <<= 1) {  // Hillis-Steele suffix scan
        for (int i = tid; i <= cap + 1; i += blockDim.x)
            suf[cur ^ 1][i] = suf[cur][i] + (i + off <= cap ? suf[cur][i + off] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int64_t row = 0;
    const int32_t lag = catchup_lag(idx, (int64_t)blockIdx.x * blockDim.x + tid, n, first, last[0], target, row);
    int32_t rank = 0;
    if (lag > 0) rank = atomicAdd(&h[lag], 1);
    __syncthreads();
    for (int i = tid + 1; i <= cap; i += blockDim.x)
        if (h[i]) base[i] = atomicAdd(&fill[i], h[i]);
    __syncthreads();
    if (lag > 0) {
        const int32_t slot = suf[cur][lag + 1] + base[lag] + rank;
        rows[slot] = (int32_t)row;
        lags[slot] = lag;
        for (int t = 0; t < nlast; ++t) last[t][row] = target;
    }
}

__global__ __launch_bounds__(256) void catchup_scatter_seg_kernel(PrepSegs) {
    const KArg(PrepSegs)* ka = (const KArg(PrepSegs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    const KArg(PrepSeg)& S = ka->seg[blockIdx.y];
    __shared__ int32_t suf[2][kMaxHistory + 2];
    __shared__ int32_t h[kMaxHistory + 1], base[kMaxHistory + 1];
    if (step_poisoned(ka->status) || S.list_cnt == nullptr) return;
    int32_t* last[2] = {S.last[0], S.last[1]};
    catchup_scatter_block(S.idx, S.n, S.first, last, S.nlast, ka->target, ka->cap, S.list_cnt,
                          S.list_cnt + (ka->cap + 1), S.list_rows, S.list_lag, suf, h, base);
}

}  // namespace

size_t coalesce_scratch_ints(int64_t key_range) { return (size_t)3 * (size_t)(key_range > 0 ? key_range : 1); }

void coalesce_bind_scratch(CoalesceWs& ws, int32_t* scratch, int64_t key_range) {
    const int64_t r = key_range > 0 ? key_range : 1;
    ws.cnt = scratch;
    ws.first = scratch ? scratch + r : nullptr;
    ws.fill = scratch ? scratch + 2 * r : nullptr;
    ws.key_range = key_range;
}

int launch_coalesce_count(const int64_t* idx, int64_t n, int64_t table_rows, CoalesceWs& ws, hipStream_t s) {
    PrepSegs ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.count = 1;
    ps.seg[0].idx = idx;
    ps.seg[0].n = n;
    ps.seg[0].cnt = ws.cnt;
    ps.seg[0].first = ws.first;
    const CoalesceWs* const wss[2] = {&ws, nullptr};
    const int64_t rows[2] = {table_rows, 0};
    return launch_prepare_segs(ps, wss, rows, s);
}

int launch_coalesce_group(const int64_t* idx, int64_t n, int64_t table_rows, CoalesceWs& ws, hipStream_t s) {
    if (n <= 0) {
        TTAMM_HIP(hipMemsetAsync(ws.n_unique, 0, sizeof(int32_t), s));
        return TTAMM_OK;
    }
    const unsigned g = (unsigned)ceil_div(n, 256);
    // segment scan over positions (first-occurrence order) or over the key range (sorted)
    const int64_t entries = ws.sorted ? table_rows : n;
    const int64_t tiles = ceil_div(entries, 256);
    TTAMM_REQUIRE(tiles <= std::max<int64_t>(n, 257), "coalesce: tile scratch too small");
    hipLaunchKernelGGL(co_tile_sum_kernel, dim3((unsigned)tiles), dim3(256), 0, s, entries, ws.sorted, idx, ws.cnt,
                       ws.first, ws.lead_cnt, ws.seglong);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_tile_scan_kernel, dim3(1), dim3(1024), 0, s, tiles, ws.lead_cnt, ws.seglong, ws.seg_start,
                       ws.n_unique);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_tile_write_kernel, dim3((unsigned)tiles), dim3(256), 0, s, entries, ws.sorted, idx, ws.cnt,
                       ws.first, ws.lead_cnt, ws.seglong, ws.lead, ws.seg_start);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_fill_kernel, dim3(g), dim3(256), 0, s, idx, n, ws.sorted, ws.lead, ws.first, ws.fill,
                       ws.seg_start, ws.vals_tmp, ws.keys_out, ws.lead_cnt);
    TTAMM_LAUNCH_CHECK();
    // segments longer than kOrderSmall: their ids in `lead` (free again), their count in
    // lead_cnt[0] (zeroed by co_fill)
    hipLaunchKernelGGL(co_order_small_kernel, dim3(g), dim3(256), 0, s, ws, ws.lead, ws.lead_cnt);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_order_big_kernel, dim3(256), dim3(256), 0, s, ws, ws.lead, ws.lead_cnt);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

int launch_coalesce(const int64_t* idx, int64_t n, int64_t table_rows, CoalesceWs& ws, hipStream_t s) {
    int rc;
    if ((rc = launch_coalesce_count(idx, n, table_rows, ws, s))) return rc;
    return launch_coalesce_group(idx, n, table_rows, ws, s);
}

namespace {
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void block_exclusive_scan_kernel(const int32_t* __restrict__ in,
                                                                            int32_t* __restrict__ out, int64_t n) {
    __shared__ int32_t sc[kScanThreads];
    const int t = threadIdx.x;
    const int64_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const int64_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    int32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += in[i];
    sc[t] = sum;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {
        const int32_t a = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    int32_t run = sc[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = in[i];
        out[i] = run;
        run += v;
    }
}
}  // namespace

int launch_block_exclusive_scan(const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
    if (n <= 0) return TTAMM_OK;
    hipLaunchKernelGGL(block_exclusive_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, in, out, n);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

size_t catchup_list_ints(int64_t n, int cap) { return (size_t)2 * (cap + 1) + (size_t)2 * (n > 0 ? n : 1) + 64; }

void catchup_bind(CatchupList& cl, int32_t* ints, int64_t n, int cap) {
    cl.cnt = ints;
    cl.fill = ints ? ints + (cap + 1) : nullptr;
    cl.rows = ints ? ints + 2 * (cap + 1) + 64 : nullptr;  // 256-B aligned past the counters
    cl.lag = ints ? cl.rows + (n > 0 ? n : 1) : nullptr;
}

int launch_prepare_segs(const PrepSegs& a, const CoalesceWs* const wss[2], const int64_t table_rows[2],
                        hipStream_t s) {
    TTAMM_REQUIRE(a.count >= 1 && a.count <= 2, "prepare: one or two towers");
    int64_t most = 0;
    bool lists = false;
    for (int i = 0; i < a.count; ++i) {
        const PrepSeg& g = a.seg[i];
        const CoalesceWs* ws = wss[i];
        const int64_t rows = table_rows[i];
        TTAMM_REQUIRE(rows < (int64_t(1) << 31) && g.n < (int64_t(1) << 31) - 1, "coalesce: table or batch too large");
        TTAMM_REQUIRE(ws && ws->key_range >= rows && ws->cnt && ws->first && ws->fill && g.cnt == ws->cnt &&
                          g.first == ws->first,
                      "coalesce: per-row scratch missing");
        TTAMM_REQUIRE(!ws->sorted || rows <= 65536, "coalesce: sorted grouping needs <= 65536 keys");
        TTAMM_REQUIRE(g.idx || g.n <= 0, "prepare: bad tower");
        TTAMM_REQUIRE(!g.list_cnt || (g.list_rows && g.list_lag && g.last[0] && g.nlast >= 1 && g.nlast <= 2 &&
                                      a.cap > 1 && a.cap <= kMaxHistory),
                      "prepare: catch-up list incomplete");
        most = g.n > most ? g.n : most;
        lists = lists || g.list_cnt;
    }
    const unsigned g = (unsigned)std::max<int64_t>(1, ceil_div(most, 256));
    hipLaunchKernelGGL(co_count_seg_kernel, dim3(g, a.count), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    if (!lists || most == 0) return TTAMM_OK;
    hipLaunchKernelGGL(catchup_count_seg_kernel, dim3(g, a.count), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(catchup_scatter_seg_kernel, dim3(g, a.count), dim3(256), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

}  // namespace ttamm
