// Block counts of the persistent fused gate kernels (gate.hip): pure host arithmetic, no device
// call, so a stand-alone program can sweep it (tools/gate_plan_check.cpp).
//
// A gate block owns its CU (all of the register file, 140 KB of LDS at D = 96), so the grid is
// sized in whole slab rounds: every wave of the launch runs `rounds` 16-row slabs (one fewer where
// a tower's slab count does not divide), and the CUs that the last round would enter for a part
// of it are left to the other stream instead.  At C2 on 256 CUs (512 + 3072 slabs, 8 waves a
// block) that is 32 + 192 blocks of two rounds, not 37 + 220 blocks of which 56 run one.
#pragma once
#include <cstdint>

namespace ttamm {

constexpr int kGateMaxTowers = 2;

struct GatePlan {
    int blocks[kGateMaxTowers];  // per tower, each >= 1
    int rounds;                  // the most slabs any wave runs
};

// nslab[t] > 0: tower t's 16-row slabs; cus: the device's CUs; waves: waves per block.
//   rounds   = ceil(sum nslab / (cus waves)), one more while the towers' blocks exceed the CUs
//   blocks_t = max(1, ceil(nslab_t / (waves rounds)))
// Then: sum blocks_t <= max(cus, count) (a tower has at least a block); blocks_t waves rounds >=
// nslab_t (a wave strides blocks_t waves slabs: every slab is covered in at most `rounds` visits);
// the waves of a tower run ceil or floor of nslab_t / (blocks_t waves) slabs; and some wave runs
// exactly `rounds` (`rounds` is lowered to the largest count when the CU bound forced it past).
inline GatePlan gate_plan(const int64_t* nslab, int count, int cus, int waves) {
    GatePlan p{};
    if (cus < 1) cus = 1;
    int64_t total = 0;
    for (int t = 0; t < count; ++t) total += nslab[t];
    const int64_t per_round = (int64_t)cus * waves;
    int64_t rounds = (total + per_round - 1) / per_round;
    if (rounds < 1) rounds = 1;
    for (;;) {
        int64_t sum = 0;
        bool all_one = true;
        for (int t = 0; t < count; ++t) {
            const int64_t per_block = (int64_t)waves * rounds;
            int64_t b = (nslab[t] + per_block - 1) / per_block;
            if (b < 1) b = 1;
            if (b > 1) all_one = false;
            p.blocks[t] = (int)b;
            sum += b;
        }
        if (sum <= cus || all_one) break;
        ++rounds;
    }
    // the largest count a wave runs with these blocks (below `rounds` only after the bump above)
    int64_t most = 1;
    for (int t = 0; t < count; ++t) {
        const int64_t w = (int64_t)p.blocks[t] * waves;
        const int64_t c = (nslab[t] + w - 1) / w;
        if (c > most) most = c;
    }
    p.rounds = (int)most;
    return p;
}

}  // namespace ttamm
