// Ranking metrics on the device: the reference's per_user_metrics / compute_ranking_metrics
// (src/evaluation/metrics.py:49-71, :74-116) for every query at once, from a row of predicted ids
// (the top-k kernels' output, still in HBM) and the query's ground-truth CSR segment.
//
// ranking_metrics_kernel: one wave per query, kQueriesPerWave consecutive queries per wave, 16 waves
// per block, so a block owns a fixed chunk of kChunk = 256 queries.  Per query the wave
//   1. reads the prediction row once (lane l holds positions l, l + 64, l + 128), drops ids < 0
//      (training.py:963) and compacts the rest in order into LDS with a 64-bit ballot + popcount;
//   2. looks every kept id up in the sorted truth segment (binary search) — ballot gives the
//      relevance mask of the list, 64 positions per word; a second mask keeps only the FIRST
//      position of each relevant id (recall / precision / hit_rate count len(set(head) & truth),
//      metrics.py:59, while ndcg / map / mrr count every position, :28-46, :66-69);
//   3. with pad_with_truth and fewer than max_k ids kept, extends both masks by the number of
//      truth items not listed yet (training.py:969-972: they are appended, all relevant, all
//      distinct, so only their count matters), cut at max_k;
//   4. lane j < n_k walks the set bits below k_values[j] in order (dcg and the running precision
//      are summed left to right in fp64, discounts and ideal DCG from the host-built tables), lane
//      n_k takes the first set bit for mrr, and each writes its columns of the query's row.
// The same lanes add their columns up over the wave's queries in query order; the block adds its
// 16 waves' sums in wave order and writes one partial row per chunk.  ranking_metrics_finish_kernel
// (one block, one thread per column) adds the chunk partials in chunk order and divides by the
// count.  No float atomics anywhere: the same inputs give the same bits.
#include <cmath>

#include "kernels.h"

namespace ttamm {

namespace {

constexpr int kWaves = 16;            // waves per block
constexpr int kQueriesPerWave = 16;   // consecutive queries of one wave
constexpr int kChunk = kWaves * kQueriesPerWave;  // queries per block = per partial row
constexpr int kWords = kMetricsMaxK / 64;         // 64 list positions per mask word

struct MetricsKernelArgs {
    const int64_t* pred;
    int64_t ld_pred;
    int64_t nq;
    const int64_t* toff;
    const int64_t* tval;
    double* rows;      // per-query rows [nq, ld_rows], or null
    int64_t ld_rows;
    double* partials;  // [chunks, kMetricsMaxCols + 1]: column sums of a chunk, then its count
    int k_pred, n_k, max_k, pad;
    int ks[kMetricsMaxNk];
    double disc[kMetricsMaxK];       // 1 / log2(i + 2)
    double idcg[kMetricsMaxK + 1];   // idcg[n] = disc[0] + ... + disc[n - 1], summed in that order
};

__device__ __forceinline__ uint64_t bits_below(int n) {  // the low n bits, n clamped to [0, 64]
    return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
}

__device__ __forceinline__ bool in_sorted(const int64_t* __restrict__ v, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && v[lo] == x;
}

__global__ __launch_bounds__(kWaves * 64) void ranking_metrics_kernel(const MetricsKernelArgs a) {
    const KArg(MetricsKernelArgs)* ka = (const KArg(MetricsKernelArgs)*)(__builtin_amdgcn_kernarg_segment_ptr());
    __shared__ int64_t s_ids[kWaves][kMetricsMaxK];
    __shared__ double s_sum[kWaves][kMetricsMaxCols + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ncol = 5 * a.n_k + 1;
    const int my_k = lane < a.n_k ? ka->ks[lane] : 0;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // lane j < n_k: k_values[j]'s five; lane n_k: mrr, count
    const int64_t q0 = (int64_t)blockIdx.x * kChunk + (int64_t)w * kQueriesPerWave;
    for (int i = 0; i < kQueriesPerWave; ++i) {
        const int64_t q = q0 + i;
        if (q >= a.nq) break;  // wave-uniform
        const int64_t t_lo = a.toff[q];
        const int64_t T = a.toff[q + 1] - t_lo;
        if (T <= 0) {  // not counted: an all-zero row (metrics.py:88-90 skips the user)
            if (a.rows && lane < ncol) a.rows[q * a.ld_rows + lane] = 0.0;
            continue;
        }
        const int64_t* __restrict__ truth = a.tval + t_lo;
        // 1. the kept ids, compacted in order
        int n_valid = 0;
#pragma unroll
        for (int c = 0; c < kWords; ++c) {
            if (c * 64 < a.k_pred) {
                const int p = c * 64 + lane;
                const int64_t id = p < a.k_pred ? a.pred[q * a.ld_pred + p] : -1;
                const bool keep = id >= 0;
                const uint64_t m = __ballot(keep);
                if (keep) s_ids[w][n_valid + __popcll(m & bits_below(lane))] = id;
                n_valid += __popcll(m);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // 2. relevance of every list position below max_k, and first occurrences among the relevant
        const int listed = n_valid < a.max_k ? n_valid : a.max_k;
        uint64_t rel[kWords], fst[kWords];
#pragma unroll
        for (int c = 0; c < kWords; ++c) rel[c] = fst[c] = 0ull;
#pragma unroll
        for (int c = 0; c < kWords; ++c) {
            if (c * 64 < listed) {
                const int p = c * 64 + lane;
                const int64_t id = p < listed ? s_ids[w][p] : -1;
                const bool r = p < listed && in_sorted(truth, T, id);
                rel[c] = __ballot(r);
                bool f = r;
                if (rel[c]) {
#pragma unroll
                    for (int cc = 0; cc <= c; ++cc) {
                        uint64_t mm = rel[cc];
                        while (mm) {  // wave-uniform walk over the earlier relevant positions
                            const int j = cc * 64 + __builtin_ctzll(mm);
                            mm &= mm - 1;
                            if (j < p && s_ids[w][j] == id) f = false;
                        }
                    }
                }
                fst[c] = __ballot(f);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next query's compaction overwrites s_ids[w]
        // 3. truth items appended behind a short list
        if (a.pad && n_valid < a.max_k) {
            int distinct = 0;
#pragma unroll
            for (int c = 0; c < kWords; ++c) distinct += __popcll(fst[c]);
            const int64_t room = a.max_k - n_valid;
            const int64_t more = T - distinct < room ? T - distinct : room;
            const int end = n_valid + (int)more;
#pragma unroll
            for (int c = 0; c < kWords; ++c) {
                const uint64_t m = bits_below(end - c * 64) & ~bits_below(n_valid - c * 64);
                rel[c] |= m;
                fst[c] |= m;
            }
        }
        // 4. the columns of this query
        if (lane < a.n_k) {
            const int k = my_k;
            int hits = 0, h = 0;
            double dcg = 0.0, ap = 0.0;
#pragma unroll
            for (int c = 0; c < kWords; ++c) {
                const uint64_t head = bits_below(k - c * 64);
                hits += __popcll(fst[c] & head);
                uint64_t mm = rel[c] & head;
                while (mm) {
                    const int p = c * 64 + __builtin_ctzll(mm);
                    mm &= mm - 1;
                    ++h;
                    dcg += ka->disc[p];
                    ap += (double)h / (double)(p + 1);
                }
            }
            const int64_t tk = T < k ? T : (int64_t)k;
            const double ideal = ka->idcg[tk];
            double v[5];
            v[0] = (double)hits / (double)T;
            v[1] = (double)hits / (double)k;
            v[2] = ideal > 0.0 ? dcg / ideal : 0.0;
            v[3] = hits > 0 ? 1.0 : 0.0;
            v[4] = ap / (double)tk;
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                acc[m] += v[m];
                if (a.rows) a.rows[q * a.ld_rows + 5 * lane + m] = v[m];
            }
        } else if (lane == a.n_k) {
            double rr = 0.0;
#pragma unroll
            for (int c = kWords - 1; c >= 0; --c)
                if (rel[c]) rr = 1.0 / (double)(c * 64 + __builtin_ctzll(rel[c]) + 1);
            acc[0] += rr;
            acc[1] += 1.0;
            if (a.rows) a.rows[q * a.ld_rows + 5 * a.n_k] = rr;
        }
    }
    // the block's chunk: waves in order
    if (lane < a.n_k) {
#pragma unroll
        for (int m = 0; m < 5; ++m) s_sum[w][5 * lane + m] = acc[m];
    } else if (lane == a.n_k) {
        s_sum[w][5 * a.n_k] = acc[0];
        s_sum[w][5 * a.n_k + 1] = acc[1];
    }
    __syncthreads();
    if ((int)threadIdx.x <= ncol) {
        double s = 0.0;
        for (int ww = 0; ww < kWaves; ++ww) s += s_sum[ww][threadIdx.x];
        a.partials[(int64_t)blockIdx.x * (kMetricsMaxCols + 1) + threadIdx.x] = s;
    }
}

// summary[c] = (partials[0][c] + partials[1][c] + ...) / count for c < ncol, summary[ncol] = count
__global__ __launch_bounds__(64) void ranking_metrics_finish_kernel(const double* __restrict__ partials, int64_t chunks,
                                                                    int ncol, double* __restrict__ summary) {
    const int c = threadIdx.x;
    if (c > ncol) return;
    double s = 0.0, n = 0.0;
    for (int64_t b = 0; b < chunks; ++b) {
        s += partials[b * (kMetricsMaxCols + 1) + c];
        n += partials[b * (kMetricsMaxCols + 1) + ncol];
    }
    summary[c] = c == ncol ? n : (n > 0.0 ? s / n : 0.0);
}

__global__ __launch_bounds__(64) void ranking_metrics_zero_kernel(double* __restrict__ summary, int n) {
    if ((int)threadIdx.x < n) summary[threadIdx.x] = 0.0;
}

}  // namespace

size_t ranking_metrics_workspace_bytes(int64_t nq, int n_k) {
    if (nq < 0 || n_k < 1 || n_k > kMetricsMaxNk) return 0;
    const int64_t chunks = nq > 0 ? ceil_div(nq, kChunk) : 1;
    return align_up((size_t)chunks * (kMetricsMaxCols + 1) * sizeof(double), 256);
}

int launch_ranking_metrics(const int64_t* pred, int64_t nq, int k_pred, int64_t ld_pred, const int64_t* toff,
                           const int64_t* tval, const int32_t* ks, int n_k, int pad, double* per_user,
                           int64_t ld_per_user, double* summary, void* ws, size_t ws_bytes, hipStream_t s) {
    TTAMM_REQUIRE(n_k >= 1 && n_k <= kMetricsMaxNk, "ranking_metrics: n_k must be in [1, 8]");
    TTAMM_REQUIRE(ks != nullptr, "ranking_metrics: null k_values");
    for (int j = 0; j < n_k; ++j)
        TTAMM_REQUIRE(ks[j] >= 1 && ks[j] <= kMetricsMaxK, "ranking_metrics: every k must be in [1, 192]");
    TTAMM_REQUIRE(nq >= 0, "ranking_metrics: n_queries must not be negative");
    TTAMM_REQUIRE(k_pred >= 0 && k_pred <= kMetricsMaxK, "ranking_metrics: k_pred must be in [0, 192]");
    TTAMM_REQUIRE(ld_pred >= k_pred, "ranking_metrics: ld_pred must be at least k_pred");
    TTAMM_REQUIRE(!per_user || ld_per_user >= 5 * n_k + 1, "ranking_metrics: ld_per_user must be at least 5 n_k + 1");
    TTAMM_REQUIRE(summary && toff && ws, "ranking_metrics: summary, truth_offsets and workspace are required");
    TTAMM_REQUIRE(pred || k_pred == 0 || nq == 0, "ranking_metrics: null pred_ids");
    TTAMM_REQUIRE(ws_bytes >= ranking_metrics_workspace_bytes(nq, n_k), "ranking_metrics: workspace too small");
    const int ncol = 5 * n_k + 1;
    if (nq == 0) {
        hipLaunchKernelGGL(ranking_metrics_zero_kernel, dim3(1), dim3(64), 0, s, summary, ncol + 1);
        TTAMM_LAUNCH_CHECK();
        return TTAMM_OK;
    }
    MetricsKernelArgs a;
    a.pred = pred;
    a.ld_pred = ld_pred;
    a.nq = nq;
    a.toff = toff;
    a.tval = tval;
    a.rows = per_user;
    a.ld_rows = ld_per_user;
    a.partials = static_cast<double*>(ws);
    a.k_pred = k_pred;
    a.n_k = n_k;
    a.max_k = 0;
    a.pad = pad ? 1 : 0;
    for (int j = 0; j < kMetricsMaxNk; ++j) {
        a.ks[j] = j < n_k ? ks[j] : 0;
        if (a.ks[j] > a.max_k) a.max_k = a.ks[j];
    }
    a.idcg[0] = 0.0;
    for (int i = 0; i < kMetricsMaxK; ++i) {
        a.disc[i] = 1.0 / std::log2((double)(i + 2));
        a.idcg[i + 1] = a.idcg[i] + a.disc[i];
    }
    const int64_t chunks = ceil_div(nq, kChunk);
    TTAMM_REQUIRE(chunks <= 0x7fffffff, "ranking_metrics: too many queries for one launch");
    hipLaunchKernelGGL(ranking_metrics_kernel, dim3((unsigned)chunks), dim3(kWaves * 64), 0, s, a);
    TTAMM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ranking_metrics_finish_kernel, dim3(1), dim3(64), 0, s, a.partials, chunks, ncol, summary);
    TTAMM_LAUNCH_CHECK();
    return TTAMM_OK;
}

}  // namespace ttamm
