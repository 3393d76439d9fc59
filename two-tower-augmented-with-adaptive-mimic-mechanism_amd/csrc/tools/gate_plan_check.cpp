// Sweeps gate_plan (gate_plan.h) on the host and exits non-zero at the first violated property.
// Host code only; tests/test_gate_plan_cpu.py builds it with -fsanitize=address,undefined.
//
// For cus in {1, 8, 256, 304}, waves in {4, 7, 8}, one tower and two towers with row counts
// 1 .. 70,000 (every count below 600, then a prime stride; R_user = 1 beside R_item = 70,000):
//   1. sum blocks <= cus (at least one block per tower: <= max(cus, towers));
//   2. every slab is covered: slab s of tower t is visited by wave s mod (blocks_t waves);
//   3. within a tower the waves' slab counts differ by at most one;
//   4. the largest count equals `rounds`, and `rounds` is the least whole number of rounds,
//      ceil(sum nslab / (cus waves)), whenever the blocks of that many rounds fit the CUs.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gate_plan.h"

namespace {

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

std::vector<int64_t> row_counts() {
    std::vector<int64_t> r;
    for (int64_t x = 1; x < 600; ++x) r.push_back(x);
    for (int64_t x = 600; x <= 70000; x += 1499) r.push_back(x);  // a prime stride
    // the last one-round / first two-round totals of 8-wave blocks on 256 CUs, the largest count
    for (int64_t x : {32767, 32768, 32769, 49152, 65536, 69999, 70000}) r.push_back(x);
    return r;
}

bool check(const int64_t* R, int count, int cus, int waves) {
    int64_t nslab[ttamm::kGateMaxTowers];
    int64_t total = 0;
    for (int t = 0; t < count; ++t) total += nslab[t] = ceil_div(R[t], 16);
    const ttamm::GatePlan p = ttamm::gate_plan(nslab, count, cus, waves);
    auto fail = [&](const char* what) {
        std::fprintf(stderr, "gate_plan: %s: cus %d waves %d rows", what, cus, waves);
        for (int t = 0; t < count; ++t) std::fprintf(stderr, " %lld", (long long)R[t]);
        std::fprintf(stderr, " -> blocks");
        for (int t = 0; t < count; ++t) std::fprintf(stderr, " %d", p.blocks[t]);
        std::fprintf(stderr, " rounds %d\n", p.rounds);
        return false;
    };
    int64_t sum = 0, most = 0;
    for (int t = 0; t < count; ++t) {
        if (p.blocks[t] < 1) return fail("a tower without a block");
        sum += p.blocks[t];
        // the kernels' loop: wave w of the tower's blocks_t * waves runs slabs w, w + W, w + 2 W, ...
        const int64_t W = (int64_t)p.blocks[t] * waves;
        std::vector<int64_t> per_wave((size_t)W, 0);
        std::vector<char> seen((size_t)nslab[t], 0);
        for (int64_t w = 0; w < W; ++w)
            for (int64_t s = w; s < nslab[t]; s += W) {
                ++per_wave[(size_t)w];
                ++seen[(size_t)s];
            }
        for (int64_t s = 0; s < nslab[t]; ++s)
            if (seen[(size_t)s] != 1) return fail("a slab not covered exactly once");
        int64_t lo = per_wave[0], hi = per_wave[0];
        for (int64_t c : per_wave) {
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        if (hi - lo > 1) return fail("slab counts of a tower's waves differ by more than one");
        most = hi > most ? hi : most;
    }
    if (sum > (cus > count ? cus : count)) return fail("more blocks than CUs");
    if (most != p.rounds) return fail("the largest slab count is not `rounds`");
    const int64_t least = ceil_div(total, (int64_t)cus * waves);
    if (p.rounds < ceil_div(total, sum * waves)) return fail("fewer rounds than the slabs need");
    int64_t fit = 0;
    for (int t = 0; t < count; ++t) fit += ceil_div(nslab[t], (int64_t)waves * least);
    if (fit <= cus && p.rounds != least) return fail("more rounds than needed");
    return true;
}

}  // namespace

int main() {
    const std::vector<int64_t> rows = row_counts();
    long long cases = 0;
    for (int cus : {1, 8, 256, 304})
        for (int waves : {4, 7, 8}) {
            for (int64_t r : rows) {
                if (!check(&r, 1, cus, waves)) return 1;
                ++cases;
            }
            // two towers: every count beside a few partners (both orders), and the counts from
            // 600 up among themselves
            for (int64_t r : rows)
                for (int64_t other : {1, 17, 599, 8192, 49152, 70000}) {
                    const int64_t ab[2] = {r, other}, ba[2] = {other, r};
                    if (!check(ab, 2, cus, waves) || !check(ba, 2, cus, waves)) return 1;
                    cases += 2;
                }
            for (int64_t a : rows)
                for (int64_t b : rows) {
                    if (a < 600 || b < 600) continue;
                    const int64_t R[2] = {a, b};
                    if (!check(R, 2, cus, waves)) return 1;
                    ++cases;
                }
        }
    // the shipped shapes on the MI355X's 256 CUs
    {
        const int64_t c2[2] = {8192 / 16, 49152 / 16};
        const ttamm::GatePlan p = ttamm::gate_plan(c2, 2, 256, 8);
        if (p.blocks[0] != 32 || p.blocks[1] != 192 || p.rounds != 2) {
            std::fprintf(stderr, "gate_plan: C2 gives %d + %d blocks, %d rounds\n", p.blocks[0], p.blocks[1], p.rounds);
            return 1;
        }
        const int64_t c4[1] = {16384 / 16};
        const ttamm::GatePlan q = ttamm::gate_plan(c4, 1, 256, 4);
        if (q.blocks[0] != 256 || q.rounds != 1) {
            std::fprintf(stderr, "gate_plan: C4 gives %d blocks, %d rounds\n", q.blocks[0], q.rounds);
            return 1;
        }
    }
    std::printf("gate_plan: %lld cases ok\n", cases);
    return 0;
}
