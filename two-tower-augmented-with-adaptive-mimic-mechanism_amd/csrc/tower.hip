// One tower on the device (tower.h): validation, the workspace planner every entry shares, and
// the forward / backward drivers — host code that issues the gfx950 kernels of kernels.h.
//
//   tower forward                         encoders.py:221-255              (a1, a3, a4)
//     hidden Linear+ReLU+Dropout GEMMs    gathered feature rows, MFMA fp32
//     final Linear -> f ; ID gather -> e  into one [rows, 2D] "ef" buffer
//     gate GEMM 1 (ReLU), gate GEMM 2 (sigmoid, mix, mimic augment)      adaptive_mimic.py:88-95 (a2)
//   tower backward (dgrad chain grouped, then all weight grads in one launch)
#include <cstdint>
#include <cstring>
#include <string>

#include "tower.h"

namespace ttamm {

namespace {
int tower_in_dim(const ttamm_tower& T, int l) { return l == 0 ? T.feat_dim : T.linear[l - 1].out_features; }
}  // namespace

// Validate one tower against the reference's own constraints.
int validate_tower(const ttamm_tower& T, const char* name, int D, bool training) {
    std::string n(name);
    TTAMM_REQUIRE(T.id.weight, n + ": embedding table missing");
    if (training) TTAMM_REQUIRE(T.id.exp_avg && T.id.exp_avg_sq, n + ": embedding optimizer state missing");
    TTAMM_REQUIRE(T.fusion == TTAMM_FUSION_CONCAT || T.id.dim == D, n + ": embedding dim mismatch");
    TTAMM_REQUIRE(D % 4 == 0 && T.id.dim % 4 == 0, n + ": ttamm requires embedding_dim % 4 == 0");
    TTAMM_REQUIRE(T.id.rows > 0, n + ": empty embedding table");
    TTAMM_REQUIRE(T.id.rows < (int64_t(1) << 31), n + ": tables of 2^31 rows or more are not supported (int32 row keys)");
    TTAMM_REQUIRE(T.n_linear >= 0 && T.n_linear <= TTAMM_MAX_LINEAR, n + ": too many feature-encoder layers");
    TTAMM_REQUIRE(T.activation >= TTAMM_ACT_RELU && T.activation <= TTAMM_ACT_SELU, n + ": unsupported activation");
    TTAMM_REQUIRE(T.fusion >= TTAMM_FUSION_IDENTITY && T.fusion <= TTAMM_FUSION_CONCAT, n + ": unsupported fusion");
    if (T.fusion != TTAMM_FUSION_IDENTITY) {
        TTAMM_REQUIRE(T.features != nullptr && T.feat_dim > 0, n + ": fusion needs feature rows");
        TTAMM_REQUIRE(T.feat_ld >= T.feat_dim, n + ": feature row stride too small");
        // the feature rows are [id.rows, feat_ld]: the weight gradient keeps their gathered row ids as int32
        TTAMM_REQUIRE(T.id.rows < (int64_t(1) << 31), n + ": feature rows of 2^31 rows or more are not supported "
                                                          "(the weight gradient gathers them by int32 row ids)");
        TTAMM_REQUIRE(T.feat_ld % 4 == 0 && (uintptr_t)T.features % 16 == 0,
                      n + ": feature rows must be 16-byte aligned (row stride % 4 == 0)");
        if (T.features_bf16)
            TTAMM_REQUIRE(T.matmul_bf16 && T.feat_bf16_ld % 8 == 0 && T.feat_bf16_ld >= round8(T.feat_dim) &&
                              (uintptr_t)T.features_bf16 % 16 == 0,
                          n + ": bf16 feature rows need matmul_bf16, 16-byte aligned rows of >= round8(F) elements");
        if (T.features_planes)
            TTAMM_REQUIRE(!T.matmul_bf16 && T.feat_planes_ld % 8 == 0 &&
                              T.feat_planes_ld >= 48 * ceil_div(T.feat_dim, 16) && (uintptr_t)T.features_planes % 16 == 0,
                          n + ": feature planes need fp32 GEMMs and 16-byte aligned rows of >= 48 ceil(F / 16) "
                              "elements (a multiple of 8)");
        for (int l = 0; l < T.n_linear; ++l) {
            const ttamm_linear& L = T.linear[l];
            TTAMM_REQUIRE(L.weight && L.bias, n + ": linear parameters missing");
            if (training)
                TTAMM_REQUIRE(L.weight_exp_avg && L.weight_exp_avg_sq && L.bias_exp_avg && L.bias_exp_avg_sq,
                              n + ": linear optimizer state missing");
            TTAMM_REQUIRE(L.in_features == tower_in_dim(T, l), n + ": feature-encoder layer shapes do not chain");
            TTAMM_REQUIRE(L.out_features % 4 == 0, n + ": ttamm requires feature-encoder widths % 4 == 0");
        }
        const int fo = fo_dim(T);
        if (T.fusion == TTAMM_FUSION_CONCAT)
            TTAMM_REQUIRE(fo % 4 == 0, n + ": ttamm requires the feature encoder's output width % 4 == 0");
        else
            TTAMM_REQUIRE(fo == D, n + ": Feature encoder output dimension must match id embedding dimension for "
                                       "'sum' or 'gated' fusion.");
        TTAMM_REQUIRE(T.dropout >= 0.f && T.dropout < 1.f, n + ": dropout must be in [0, 1)");
    }
    if (T.fusion == TTAMM_FUSION_GATED) {
        const ttamm_linear &G1 = T.gate[0], &G2 = T.gate[1];
        TTAMM_REQUIRE(G1.weight && G1.bias && G2.weight && G2.bias, n + ": gate parameters missing");
        if (training)
            TTAMM_REQUIRE(G1.weight_exp_avg && G1.weight_exp_avg_sq && G1.bias_exp_avg && G1.bias_exp_avg_sq &&
                              G2.weight_exp_avg && G2.weight_exp_avg_sq && G2.bias_exp_avg && G2.bias_exp_avg_sq,
                          n + ": gate optimizer state missing");
        TTAMM_REQUIRE(G1.in_features == 2 * D && G2.out_features == D && G2.in_features == G1.out_features,
                      n + ": gate shapes do not match the embedding dimension");
        TTAMM_REQUIRE(G1.out_features % 4 == 0, n + ": ttamm requires the gate hidden width % 4 == 0");
    }
    if (T.fusion == TTAMM_FUSION_CONCAT) {
        const ttamm_linear& P = T.gate[0];
        TTAMM_REQUIRE(P.weight && P.bias, n + ": concat projection parameters missing");
        if (training)
            TTAMM_REQUIRE(P.weight_exp_avg && P.weight_exp_avg_sq && P.bias_exp_avg && P.bias_exp_avg_sq,
                          n + ": concat projection optimizer state missing");
        TTAMM_REQUIRE(P.in_features == efw(T) && P.out_features == D,
                      n + ": concat projection must map [e | f] (embedding dim + feature output) to the output dim");
    }
    return TTAMM_OK;
}

int validate_pair(const ttamm_step_args& A, bool training) {
    const int D = out_dim(A.user);
    int rc;
    if ((rc = validate_tower(A.user, "user_encoder", D, training))) return rc;
    if ((rc = validate_tower(A.item, "item_encoder", D, training))) return rc;
    TTAMM_REQUIRE(out_dim(A.item) == D, "User and item encoders must produce embeddings with the same dimension.");
    TTAMM_REQUIRE(A.user.matmul_bf16 == A.item.matmul_bf16, "user and item towers must share one matmul precision");
    return TTAMM_OK;
}

int validate_mimic_pair(const ttamm_step_args& A) {
    const int D = out_dim(A.user);
    if (A.mimic_enabled) {
        TTAMM_REQUIRE(A.user.mimic.weight && A.item.mimic.weight, "mimic tables missing");
        TTAMM_REQUIRE(A.user.mimic.dim == D && A.item.mimic.dim == D &&
                          A.user.mimic.rows == A.user.id.rows && A.item.mimic.rows == A.item.id.rows,
                      "Adaptive mimic requires user and item embedding dimensions to match.");
    }
    return TTAMM_OK;
}

// The replicated-weight gradient arena: per tower (user, item) the feature-encoder layers'
// weight, bias, then the gate's, each piece padded to 64 floats (256 B).
inline size_t pad64(size_t n) { return (n + 63) / 64 * 64; }
size_t tower_grad_floats(const ttamm_tower& T) {
    size_t n = 0;
    if (T.fusion == TTAMM_FUSION_IDENTITY) return 0;
    for (int l = 0; l < T.n_linear; ++l)
        n += pad64((size_t)T.linear[l].out_features * T.linear[l].in_features) + pad64(T.linear[l].out_features);
    for (int q = 0; q < fusion_linears(T); ++q)
        n += pad64((size_t)T.gate[q].out_features * T.gate[q].in_features) + pad64(T.gate[q].out_features);
    return n;
}
void carve_grads(const ttamm_tower& T, TowerWs& w, float*& cur) {
    if (T.fusion == TTAMM_FUSION_IDENTITY) return;
    for (int l = 0; l < T.n_linear; ++l) {
        w.gw[l] = cur;
        cur += pad64((size_t)T.linear[l].out_features * T.linear[l].in_features);
        w.gb[l] = cur;
        cur += pad64(T.linear[l].out_features);
    }
    for (int q = 0; q < fusion_linears(T); ++q) {
            w.ggw[q] = cur;
            cur += pad64((size_t)T.gate[q].out_features * T.gate[q].in_features);
            w.ggb[q] = cur;
            cur += pad64(T.gate[q].out_features);
        }
}

// The weight-gradient problems of one tower (tower_backward's list), for the split choice.
int wgrad_shapes(const ttamm_tower& T, int64_t R, WgradShape* out) {
    int n = 0;
    if (T.fusion == TTAMM_FUSION_IDENTITY) return 0;
    for (int l = 0; l < T.n_linear; ++l) out[n++] = WgradShape{R, T.linear[l].out_features, T.linear[l].in_features};
    for (int q = 0; q < fusion_linears(T); ++q) out[n++] = WgradShape{R, T.gate[q].out_features, T.gate[q].in_features};
    return n;
}

namespace {
// the split-K slabs of a tower's weight gradients (w.wgrad_rps chosen before): the feature
// encoder's layers, then the fusion's
void plan_slabs(Arena& ar, const ttamm_tower& T, int64_t R, TowerWs& w) {
    if (T.fusion == TTAMM_FUSION_IDENTITY) return;
    for (int i = 0; i < T.n_linear + fusion_linears(T); ++i) {
        const ttamm_linear& L = i < T.n_linear ? T.linear[i] : T.gate[i - T.n_linear];
        w.slab[i < T.n_linear ? i : TTAMM_MAX_LINEAR + i - T.n_linear] = ar.take<float>(
            wgrad_slab_floats((int)R, L.out_features, L.in_features, w.wgrad_rps[wgrad_class(L.out_features)]));
    }
}
}  // namespace

void plan_tower(Arena& ar, const ttamm_tower& T, int64_t R, const TowerPlan& o, TowerWs& w) {
    const int D = out_dim(T);
    w.R = R;
    w.idx_own = ar.take<int64_t>(R);
    for (int l = 0; l + 1 < T.n_linear; ++l) {
        const size_t n = (size_t)R * T.linear[l].out_features;
        w.hid[l] = ar.take<float>(n);
        if (!o.backward) continue;
        w.dhid[l] = ar.take<float>(n);
        if (T.activation != TTAMM_ACT_RELU) {
            w.pre[l] = ar.take<float>(n);
            if (T.dropout > 0.f) w.mask[l] = ar.take<uint8_t>(n);
        }
    }
    if (uses_ef(T)) {
        w.ef = ar.take<float>((size_t)R * efw(T));
        if (o.backward) w.dEF = ar.take<float>((size_t)R * efw(T));
    } else {
        w.e = ar.take<float>((size_t)R * D);
        if (T.fusion == TTAMM_FUSION_SUM || o.f_any) w.f = ar.take<float>((size_t)R * D);
    }
    if (T.fusion == TTAMM_FUSION_GATED) {
        const int Hg = T.gate[0].out_features;
        w.z = ar.take<float>((size_t)R * Hg);
        if (o.backward) w.dz = ar.take<float>((size_t)R * Hg);
        w.g = ar.take<float>((size_t)R * D);
        if (o.backward) w.dq = ar.take<float>((size_t)R * D);
        const int np = T.matmul_bf16 ? 1 : 3;
        if (o.gw16 && gate16_supported(D, Hg, np)) w.gw16 = ar.take<uint16_t>((size_t)gate16_image_elems(D, Hg, np));
    }
    if (o.io & IO_T) {
        w.t = ar.take<float>((size_t)R * D);
        w.a = o.mimic ? ar.take<float>((size_t)R * D) : nullptr;
        w.t_ld = D;
    }
    if (o.io & IO_AUG) w.aug = ar.take<float>((size_t)R * D);
    if (o.io & IO_DT) {
        w.dT_own = ar.take<float>((size_t)R * D);
        w.dT = w.dT_own;
        w.dT_ld = D;
        w.dA_own = o.mimic ? ar.take<float>((size_t)o.dA_rows * D) : nullptr;
        w.dA = w.dA_own;
        w.dA_ld = D;
        w.dA_split = o.dA_rows;
    }
    if (o.backward) plan_slabs(ar, T, R, w);
    if (needs_wpad(T)) w.wpad = ar.take<float>((size_t)T.linear[0].out_features * round4(T.linear[0].in_features));
    if (o.w16 && uses_w16(T))
        w.w16 = ar.take<uint16_t>((size_t)T.linear[0].out_features * round8(T.linear[0].in_features));
    if (o.claim_marks && T.id.max_norm > 0.0) w.renorm_mark = ar.take<int32_t>(T.id.rows);
}

namespace {
GemmProblem gp_base() {
    GemmProblem p;
    std::memset(&p, 0, sizeof(p));
    p.keep_prob = 1.f;
    p.inv_keep = 1.f;
    p.a_ones_col = -1;
    return p;
}

struct Batcher {
    GemmBatch b;
    Batcher() { std::memset(&b, 0, sizeof(b)); }
    void add(const GemmProblem& p) { b.p[b.count++] = p; }
    int run(hipStream_t s) {
        if (b.count == 0) return TTAMM_OK;
        int rc = launch_gemm(b, s);
        std::memset(&b, 0, sizeof(b));
        return rc;
    }
};

// Dropout RNG words: key = seed; counter words 2,3 = step counter / (domain | tower | layer)
void set_dropout(GemmProblem& p, const ttamm_tower& T, const ttamm_batch& bt, int tower_id, int layer,
                 const uint8_t* mask) {
    const float pdrop = T.dropout;
    p.keep_prob = 1.0f - pdrop;
    // torch computes noise/(1-p) in fp32: 1.f / (1.f - p)
    p.inv_keep = pdrop > 0.f ? 1.0f / (1.0f - pdrop) : 1.0f;
    p.keep_mask = mask;
    p.rng_k0 = (uint32_t)bt.seed;
    p.rng_k1 = (uint32_t)(bt.seed >> 32);
    p.rng_c2 = (uint32_t)bt.counter;
    p.rng_c3 = RNG_DROPOUT | ((uint32_t)tower_id << 24) | ((uint32_t)layer << 20) |
               ((uint32_t)(bt.counter >> 32) & 0xFFFFFu);
}

void set_keys(GemmProblem& p, const TowerWs& w) {
    p.row_key = w.row_key;
    p.key_base0 = w.key_base0;
    p.key_base1 = w.key_base1;
    p.key_split = w.key_split;
}

// ---- fused gate (gate.hip) ------------------------------------------------------------------
// Used when every gated tower of a grouped launch has a supported D == Hg: fp32 towers gate.hip
// (D in {32, 64, 96, 128}), bf16 towers gate16.hip (D in {128, 256}); any other configuration runs
// the generic GEMM path.  TTAMM_GENERIC_GATE=1 forces the generic path (the tests run both).
bool generic_gate_forced() {
    const char* v = product_env("TTAMM_GENERIC_GATE");
    return v && v[0] == '1';
}
}  // namespace

// Whether the gated towers of a grouped launch all run on one fused gate kernel, and which: their
// common hidden width and form (planes 0: gate.hip, 1 / 3: gate16.hip).  has16[k]: tower k has
// gate16 weight images (plan() gives a gated tower some exactly when gate16_supported).
bool gate_choice(const ttamm_tower* const* T, const bool* has16, int ntowers, int D, int& hg, int& planes) {
    hg = planes = -1;
    if (generic_gate_forced()) return false;
    // TTAMM_GATE16_SPLIT=1: fp32 towers at D = 96 on gate16.hip's split-bf16 form instead of gate.hip
    // (fp32 MFMA).  Measured slower at C2 (forward 71 vs 61 us, backward 72 vs 70, step 0.695 vs
    // 0.655 ms, profiles/r05_s20_gate16_split.txt): the kernels are latency-bound, not MFMA-bound
    const char* e16 = dev_env("TTAMM_GATE16_SPLIT");
    const bool split16 = e16 && e16[0] == '1';
    for (int k = 0; k < ntowers; ++k) {
        const ttamm_tower& t = *T[k];
        if (t.fusion != TTAMM_FUSION_GATED) continue;
        const int h = t.gate[0].out_features;
        int np;
        if (t.matmul_bf16) {
            if (!(gate16_supported(D, h, 1) && has16[k])) return false;
            np = 1;
        } else if (split16 && gate16_supported(D, h, 3) && has16[k]) {
            np = 3;
        } else if (gate_fused_supported(D, h)) {
            np = 0;
        } else {
            return false;
        }
        if ((hg >= 0 && h != hg) || (planes >= 0 && np != planes)) return false;
        hg = h;
        planes = np;
    }
    return hg >= 0;
}

namespace {
bool gate_group(const ttamm_tower* const* T, TowerWs* const* W, int ntowers, int D, bool mimic, GateArgs& ga) {
    std::memset(&ga, 0, sizeof(ga));
    bool has16[2] = {};
    for (int k = 0; k < ntowers; ++k) has16[k] = W[k]->gw16 != nullptr;
    int hg, planes;
    if (!gate_choice(T, has16, ntowers, D, hg, planes)) return false;
    ga.planes = planes;
    ga.images_ready = 1;
    for (int k = 0; k < ntowers; ++k) {
        const ttamm_tower& t = *T[k];
        const TowerWs& w = *W[k];
        if (t.fusion != TTAMM_FUSION_GATED || w.R <= 0) continue;
        GateTower& g = ga.tw[ga.count++];
        g.R = w.R;
        g.ef = w.ef;
        g.G1 = t.gate[0].weight;
        g.c1 = t.gate[0].bias;
        g.G2 = t.gate[1].weight;
        g.c2 = t.gate[1].bias;
        g.z = w.z;
        g.g = w.g;
        g.t = w.t;
        g.a = w.a;
        g.ld_t = w.t_ld;
        g.table = mimic ? t.mimic.weight : nullptr;
        g.idx = w.idx;
        g.aug = w.aug;
        g.dT = w.dT;
        g.ld_dT = w.dT_ld;
        g.dq = w.dq;
        g.dz = w.dz;
        g.dEF = w.dEF;
        g.xu = w.xu;
        g.w16 = w.gw16;
        if (!w.gw16_ready) ga.images_ready = 0;
    }
    ga.D = D;
    ga.HG = hg;
    return true;
}

// compact exchange rows (TowerWs::xu) are addressed by the fused gate kernels only
int require_fused_for_units(const ttamm_tower* const* T, TowerWs* const* W, int ntowers, bool fused_gate) {
    for (int k = 0; k < ntowers; ++k)
        TTAMM_REQUIRE(!W[k]->xu || (T[k]->fusion == TTAMM_FUSION_GATED && fused_gate),
                      "compact exchange rows (exchange_counts) need the item tower on the fused gate kernels "
                      "(ttamm_exchange_compact_supported)");
    return TTAMM_OK;
}

// ---- forward -------------------------------------------------------------------------------
// TTAMM_GATE_OUT_EPILOGUE=1: the generic gate's sigmoid mix / mimic augment in the second gate
// GEMM's epilogue (EPI_GATE_OUT) instead of gate_mix_kernel after an EPI_STORE launch
bool gate_out_epilogue() {
    static const bool on = dev_env("TTAMM_GATE_OUT_EPILOGUE") != nullptr;
    return on;
}
int forward_fusion(const ttamm_tower* T[2], TowerWs* W[2], int D, bool mimic, hipStream_t s, int ntowers);
}  // namespace

int tower_forward(const ttamm_tower* T[2], TowerWs* W[2], const ttamm_batch& bt, int D, bool mimic, hipStream_t s,
                  int ntowers, void* const* l0_events, int part, hipEvent_t after_l0) {
    int rc;
    if (part & FWD_GATHER) {
        // ID rows -> e (ef[:, :D] when gated): both towers' gathers in one launch
        GatherSegs gs;
        gs.count = 0;
        for (int k = 0; k < ntowers; ++k) {
            const ttamm_tower& t = *T[k];
            TowerWs& w = *W[k];
            if (t.id.max_norm > 0.0 && w.R > 0 && w.row_key && w.renorm_key_split > 0) {
                // sharded owner: every requester's positives (keys < global batch) are the reference's
                // first item lookup (training.py:750), the negatives its second (:776)
                for (int ph = 0; ph < 2; ++ph)
                    if ((rc = launch_renorm_rows(t.id.weight, t.id.rows, t.id.dim, w.idx, w.R, t.id.max_norm, w.renorm_mark,
                                                 w.renorm_tag + ph, s, w.row_key, w.renorm_key_split, ph)))
                        return rc;
            } else if (t.id.max_norm > 0.0 && w.R > 0) {  // nn.Embedding max_norm: renorm, then look up
                const int64_t split = w.renorm_split > 0 && w.renorm_split < w.R ? w.renorm_split : w.R;
                if ((rc = launch_renorm_rows(t.id.weight, t.id.rows, t.id.dim, w.idx, split, t.id.max_norm, w.renorm_mark,
                                             w.renorm_tag, s)))
                    return rc;
                if (split < w.R &&
                    (rc = launch_renorm_rows(t.id.weight, t.id.rows, t.id.dim, w.idx + split, w.R - split, t.id.max_norm,
                                             w.renorm_mark, w.renorm_tag + 1, s)))
                    return rc;
            }
            float* dst = uses_ef(t) ? w.ef : w.e;
            const int64_t ld = uses_ef(t) ? efw(t) : t.id.dim;
            gs.seg[gs.count++] = GatherSeg{t.id.weight, t.id.rows, t.id.dim, w.idx, w.R, dst, ld};
        }
        if ((rc = launch_gather_rows_segs(gs, s))) return rc;
    }
    if (part & FWD_FEAT) {
        for (int k = 0; k < ntowers; ++k) {
            const ttamm_tower& t = *T[k];
            TowerWs& w = *W[k];
            if (t.fusion != TTAMM_FUSION_IDENTITY && t.n_linear == 0 && w.R > 0) {
                // identity feature encoder (encoders.py:114-119): f = the feature row
                const int64_t ld = uses_ef(t) ? efw(t) : t.id.dim;
                float* fdst = uses_ef(t) ? w.ef + t.id.dim : w.f;
                if ((rc = launch_add_rows(t.features, t.feat_ld, nullptr, 0, w.R, fo_dim(t), fdst, ld, s, w.fidx)))
                    return rc;
            }
        }
        // feature encoder layers
        int maxL = 0;
        for (int k = 0; k < ntowers; ++k)
            if (T[k]->fusion != TTAMM_FUSION_IDENTITY) maxL = T[k]->n_linear > maxL ? T[k]->n_linear : maxL;
        for (int l = 0; l < maxL; ++l) {
            Batcher bb;
            PadSegs pads;  // first-layer weights padded to 16-B rows, both towers in one launch
            pads.count = 0;
            for (int k = 0; k < ntowers; ++k) {
                const ttamm_tower& t = *T[k];
                TowerWs& w = *W[k];
                if (t.fusion == TTAMM_FUSION_IDENTITY || l >= t.n_linear) continue;
                const ttamm_linear& L = t.linear[l];
                GemmProblem p = gp_base();
                p.bf16 = t.matmul_bf16;
                if (l == 0) {
                    p.A = t.features;
                    p.a_idx = w.fidx;
                    p.lda = t.feat_ld;
                } else {
                    p.A = w.hid[l - 1];
                    p.lda = t.linear[l - 1].out_features;
                }
                p.B = L.weight;
                p.ldb = L.in_features;
                if (l == 0 && w.w16) {  // bf16 operands in memory (C5 layer 1)
                    const int kp = round8(L.in_features);
                    if ((rc = launch_to_bf16(L.weight, L.out_features, L.in_features, L.in_features, w.w16, kp, s)))
                        return rc;
                    p.A16 = t.features_bf16;
                    p.lda = t.feat_bf16_ld;
                    p.B16 = w.w16;
                    p.ldb = kp;
                } else if (l == 0 && w.wpad) {
                    pads.seg[pads.count++] = PadSeg{L.weight, L.out_features, L.in_features, L.in_features, w.wpad,
                                                    round4(L.in_features)};
                    p.B = w.wpad;
                    p.ldb = round4(L.in_features);
                }
                p.b_kn = 0;
                p.M = (int)w.R;
                p.N = L.out_features;
                p.K = L.in_features;
                // the feature rows and the padded weight are zero beyond F: run K to the padded
                // width so every k-tile is whole (fast GEMM path)
                if (l == 0 && w.wpad && t.feat_ld >= round4(L.in_features)) p.K = round4(L.in_features);
                if (l == 0 && w.w16) p.K = round8(L.in_features);  // both operands zero beyond F
                // pre-split feature rows (ttamm_tower.features_planes): zero beyond F up to whole
                // 16-k chunks, so K may run to the padded width
                if (l == 0 && t.features_planes && !t.matmul_bf16 && p.K <= 16 * (t.feat_planes_ld / 48)) {
                    p.A3p = t.features_planes;
                    p.lda3 = t.feat_planes_ld;
                }
                p.bias = L.bias;
                if (l + 1 < t.n_linear) {
                    p.epi = EPI_HIDDEN;
                    p.C = w.hid[l];
                    p.ldc = L.out_features;
                    const uint8_t* injected = w.role == ROLE_USER ? bt.user_keep_mask[l] : bt.item_keep_mask[l];
                    set_dropout(p, t, bt, w.role, l, injected);
                    set_keys(p, w);
                    p.act = t.activation;
                    if (t.activation != TTAMM_ACT_RELU) {  // the backward's inputs
                        p.pre = w.pre[l];
                        if (t.dropout > 0.f && injected == nullptr) p.mask_out = w.mask[l];
                        w.keep[l] = injected ? injected : w.mask[l];
                    }
                } else {
                    p.epi = EPI_STORE;
                    if (uses_ef(t)) {
                        p.C = w.ef + t.id.dim;
                        p.ldc = efw(t);
                    } else {
                        p.C = w.f;
                        p.ldc = D;
                    }
                }
                bb.add(p);
            }
            if ((rc = launch_pad_rows_segs(pads, s))) return rc;
            const bool timed = l == 0 && l0_events && l0_events[0] && l0_events[1];
            if (timed) TTAMM_HIP(hipEventRecord((hipEvent_t)l0_events[0], s));
            if ((rc = bb.run(s))) return rc;
            if (timed) TTAMM_HIP(hipEventRecord((hipEvent_t)l0_events[1], s));
            if (l == 0 && after_l0) TTAMM_HIP(hipEventRecord(after_l0, s));
        }
    }
    return part & FWD_FUSION ? forward_fusion(T, W, D, mimic, s, ntowers) : TTAMM_OK;
}

namespace {
// part FWD_FUSION: the gate (fused kernel or two GEMMs + mix), the concat projection, or the combine
int forward_fusion(const ttamm_tower* T[2], TowerWs* W[2], int D, bool mimic, hipStream_t s, int ntowers) {
    int rc;
    GateArgs ga;
    const bool fused_gate = gate_group(T, W, ntowers, D, mimic, ga);
    if ((rc = require_fused_for_units(T, W, ntowers, fused_gate))) return rc;
    if (fused_gate && ga.count > 0) {
        if ((rc = launch_gate(ga, false, s))) return rc;
        for (int k = 0; k < ntowers; ++k) W[k]->gw16_ready = W[k]->gw16 != nullptr;
    }
    Batcher g1, g2, gc;
    for (int k = 0; k < ntowers; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        const float* table = mimic ? t.mimic.weight : nullptr;
        if (t.fusion == TTAMM_FUSION_CONCAT) {  // t = [e | f] P^T + b (encoders.py:242-244)
            GemmProblem p = gp_base();
            p.bf16 = t.matmul_bf16;
            p.A = w.ef;
            p.lda = efw(t);
            p.B = t.gate[0].weight;
            p.ldb = efw(t);
            p.M = (int)w.R;
            p.N = D;
            p.K = efw(t);
            p.bias = t.gate[0].bias;
            p.epi = EPI_STORE;
            p.C = w.t;
            p.ldc = w.t_ld;
            gc.add(p);
            continue;
        }
        if (t.fusion == TTAMM_FUSION_GATED) {
            if (fused_gate) continue;
            const int Hg = t.gate[0].out_features;
            GemmProblem p = gp_base();
            p.bf16 = t.matmul_bf16;
            p.A = w.ef;
            p.lda = 2 * D;
            p.B = t.gate[0].weight;
            p.ldb = 2 * D;
            p.M = (int)w.R;
            p.N = Hg;
            p.K = 2 * D;
            p.bias = t.gate[0].bias;
            p.epi = EPI_GATE_HIDDEN;
            p.C = w.z;
            p.ldc = Hg;
            g1.add(p);
            GemmProblem q = gp_base();
            q.bf16 = t.matmul_bf16;
            q.A = w.z;
            q.lda = Hg;
            q.B = t.gate[1].weight;
            q.ldb = Hg;
            q.M = (int)w.R;
            q.N = D;
            q.K = Hg;
            q.bias = t.gate[1].bias;
            if (gate_out_epilogue()) {  // TTAMM_GATE_OUT_EPILOGUE=1: the mix in the GEMM's epilogue
                q.epi = EPI_GATE_OUT;
                q.C = w.aug;
                q.ldc = D;
                q.aux0 = w.ef;
                q.ld_aux0 = 2 * D;
                q.out1 = w.g;
                q.out2 = w.t;
                q.out3 = w.a;
                q.table = table;
                q.idx = w.idx;
                q.ld_out = D;
                q.ld_out2 = w.t_ld;
            } else {  // the pre-activation into g; gate_mix_kernel below (rows.hip)
                q.epi = EPI_STORE;
                q.C = w.g;
                q.ldc = D;
            }
            g2.add(q);
        } else {
            if ((rc = launch_combine(w.e, D, t.fusion == TTAMM_FUSION_SUM ? w.f : nullptr, D, table, t.mimic.rows, w.idx,
                                     w.R, D, w.t, w.a, w.t_ld, w.aug, s)))
                return rc;
        }
    }
    if ((rc = g1.run(s))) return rc;
    if ((rc = g2.run(s))) return rc;
    if (!gate_out_epilogue() && !fused_gate) {
        for (int k = 0; k < ntowers; ++k) {
            const ttamm_tower& t = *T[k];
            TowerWs& w = *W[k];
            if (t.fusion != TTAMM_FUSION_GATED) continue;
            if ((rc = launch_gate_mix(w.g, w.ef, mimic ? t.mimic.weight : nullptr, w.idx, w.R, D, w.t, w.a, w.t_ld, w.aug, s)))
                return rc;
        }
    }
    if ((rc = gc.run(s))) return rc;
    for (int k = 0; k < ntowers; ++k) {  // concat: a = A[idx], aug = t + a (in place on t)
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (t.fusion != TTAMM_FUSION_CONCAT) continue;
        if ((rc = launch_combine(w.t, w.t_ld, nullptr, D, mimic ? t.mimic.weight : nullptr, t.mimic.rows, w.idx, w.R,
                                 D, w.t, w.a, w.t_ld, w.aug, s)))
            return rc;
    }
    return TTAMM_OK;
}

// ---- backward ------------------------------------------------------------------------------
int tower_wgrads(const ttamm_tower* T[2], TowerWs* W[2], int D, hipStream_t s, int ntowers, void* const* wg_events,
                 const DenseTail* dense);
}  // namespace

int tower_backward(const ttamm_tower* T[2], TowerWs* W[2], int D, hipStream_t s, int ntowers,
                   void* const* wg_events, int part, const DenseTail* dense) {
    int rc;
    if (part & BWD_GATE) {
    // gate: dq, dz, dEF
    GateArgs ga;
    const bool fused_gate = gate_group(T, W, ntowers, D, false, ga);
    if ((rc = require_fused_for_units(T, W, ntowers, fused_gate))) return rc;
    if (fused_gate && ga.count > 0)
        if ((rc = launch_gate(ga, true, s))) return rc;
    Batcher b1, b2;
    for (int k = 0; k < ntowers; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (t.fusion != TTAMM_FUSION_GATED || fused_gate) continue;
        const int Hg = t.gate[0].out_features;
        if ((rc = launch_gate_dq(w.dT, w.dT_ld, w.ef, w.g, w.R, D, w.dq, s))) return rc;
        GemmProblem p = gp_base();  // dz = (dq . G2) * (z > 0)
        p.bf16 = t.matmul_bf16;
        p.A = w.dq;
        p.lda = D;
        p.B = t.gate[1].weight;  // [D, Hg] = [K, N]
        p.ldb = Hg;
        p.b_kn = 1;
        p.M = (int)w.R;
        p.N = Hg;
        p.K = D;
        p.epi = EPI_DGRAD_RELU;
        p.C = w.dz;
        p.ldc = Hg;
        p.aux0 = w.z;
        p.ld_aux0 = Hg;
        b1.add(p);
        GemmProblem q = gp_base();  // [de | df] = dz . G1 + gate-mix terms
        q.bf16 = t.matmul_bf16;
        q.A = w.dz;
        q.lda = Hg;
        q.B = t.gate[0].weight;  // [Hg, 2D] = [K, N]
        q.ldb = 2 * D;
        q.b_kn = 1;
        q.M = (int)w.R;
        q.N = 2 * D;
        q.K = Hg;
        q.epi = EPI_DGRAD_GATE_EF;
        q.C = w.dEF;
        q.ldc = 2 * D;
        q.aux1 = w.dT;
        q.ld_aux1 = w.dT_ld;
        q.aux2 = w.g;
        q.ld_aux2 = D;
        b2.add(q);
    }
    for (int k = 0; k < ntowers; ++k) {  // concat: d[e | f] = dT P
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (t.fusion != TTAMM_FUSION_CONCAT) continue;
        GemmProblem q = gp_base();
        q.bf16 = t.matmul_bf16;
        q.A = w.dT;
        q.lda = w.dT_ld;
        q.B = t.gate[0].weight;  // [D, Did + Fo] = [K, N]
        q.ldb = efw(t);
        q.b_kn = 1;
        q.M = (int)w.R;
        q.N = efw(t);
        q.K = D;
        q.epi = EPI_STORE;
        q.C = w.dEF;
        q.ldc = efw(t);
        b2.add(q);
    }
    if ((rc = b1.run(s))) return rc;
    if ((rc = b2.run(s))) return rc;
    }
    if (!(part & BWD_MLP)) return TTAMM_OK;
    // MLP dgrad chain (layers L-1 .. 1)
    int maxL = 0;
    for (int k = 0; k < ntowers; ++k)
        if (T[k]->fusion != TTAMM_FUSION_IDENTITY) maxL = T[k]->n_linear > maxL ? T[k]->n_linear : maxL;
    for (int step = 0; step + 1 < maxL; ++step) {
        Batcher bb;
        for (int k = 0; k < ntowers; ++k) {
            const ttamm_tower& t = *T[k];
            TowerWs& w = *W[k];
            if (t.fusion == TTAMM_FUSION_IDENTITY) continue;
            const int l = t.n_linear - 1 - step;  // layer whose input grad we compute
            if (l < 1) continue;
            const ttamm_linear& L = t.linear[l];
            GemmProblem p = gp_base();
            p.bf16 = t.matmul_bf16;
            if (l == t.n_linear - 1) {
                p.A = uses_ef(t) ? w.dEF + t.id.dim : w.dT;
                p.lda = uses_ef(t) ? efw(t) : w.dT_ld;
            } else {
                p.A = w.dhid[l];
                p.lda = L.out_features;
            }
            p.B = L.weight;  // [out, in] = [K, N]
            p.ldb = L.in_features;
            p.b_kn = 1;
            p.M = (int)w.R;
            p.N = L.in_features;
            p.K = L.out_features;
            p.epi = EPI_DGRAD_HIDDEN;
            p.C = w.dhid[l - 1];
            p.ldc = L.in_features;
            p.aux0 = w.hid[l - 1];
            p.ld_aux0 = L.in_features;
            const float pdrop = t.dropout;
            p.inv_keep = pdrop > 0.f ? 1.0f / (1.0f - pdrop) : 1.0f;
            p.act = t.activation;
            if (t.activation != TTAMM_ACT_RELU) {  // act'(pre-activation), the forward's keep bytes
                p.aux0 = w.pre[l - 1];
                p.keep_prob = 1.0f - pdrop;
                p.keep_mask = pdrop > 0.f ? w.keep[l - 1] : nullptr;
            }
            bb.add(p);
        }
        if ((rc = bb.run(s))) return rc;
    }
    return tower_wgrads(T, W, D, s, ntowers, wg_events, dense);
}

namespace {
// dW = dY^T X ([M, N]) and db = sum dY over the tower's rows, into the gradient arena through `slab`
WgradProblem wgrad_problem(const ttamm_tower& t, const TowerWs& w, const float* dY, int64_t ld_dy, const float* X,
                           int64_t ld_x, int M, int N, float* grad_w, float* grad_b, float* slab) {
    WgradProblem p{};
    p.bf16 = t.matmul_bf16;
    p.dY = dY, p.ld_dy = ld_dy;
    p.X = X, p.ld_x = ld_x;
    p.R = (int)w.R, p.M = M, p.N = N;
    p.grad_w = grad_w, p.grad_b = grad_b, p.slab = slab;
    p.rows_per_split = w.wgrad_rps[wgrad_class(M)];
    return p;
}

// all weight gradients in one grouped launch; dense: each Linear's AdamW update with its reduce
int tower_wgrads(const ttamm_tower* T[2], TowerWs* W[2], int D, hipStream_t s, int ntowers, void* const* wg_events,
                 const DenseTail* dense) {
    WgradBatch wb;
    std::memset(&wb, 0, sizeof(wb));
    WgradTail tail;
    std::memset(&tail, 0, sizeof(tail));
    // the Linear whose gradient is problem wb.count (called right before the problem is added)
    auto owner = [&](const ttamm_linear& L) {
        tail.t[wb.count] = WgradTailParam{L.weight, L.weight_exp_avg, L.weight_exp_avg_sq,
                                          L.bias,   L.bias_exp_avg,   L.bias_exp_avg_sq};
    };
    for (int k = 0; k < ntowers; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (t.fusion == TTAMM_FUSION_IDENTITY) continue;
        float* const* gslab = w.slab + TTAMM_MAX_LINEAR;
        if (t.fusion == TTAMM_FUSION_GATED) {
            const int Hg = t.gate[0].out_features;
            owner(t.gate[1]);
            wb.p[wb.count++] = wgrad_problem(t, w, w.dq, D, w.z, Hg, D, Hg, w.ggw[1], w.ggb[1], gslab[1]);
            owner(t.gate[0]);
            wb.p[wb.count++] = wgrad_problem(t, w, w.dz, Hg, w.ef, 2 * D, Hg, 2 * D, w.ggw[0], w.ggb[0], gslab[0]);
        }
        if (t.fusion == TTAMM_FUSION_CONCAT) {  // dP = dT^T [e | f], db = sum dT
            owner(t.gate[0]);
            wb.p[wb.count++] =
                wgrad_problem(t, w, w.dT, w.dT_ld, w.ef, efw(t), D, efw(t), w.ggw[0], w.ggb[0], gslab[0]);
        }
        for (int l = t.n_linear - 1; l >= 0; --l) {
            const ttamm_linear& L = t.linear[l];
            const bool last = l == t.n_linear - 1;
            const float* dY = !last ? w.dhid[l] : uses_ef(t) ? w.dEF + t.id.dim : w.dT;
            const int64_t ld_dy = !last ? L.out_features : uses_ef(t) ? efw(t) : w.dT_ld;
            WgradProblem p = l == 0 ? wgrad_problem(t, w, dY, ld_dy, t.features, t.feat_ld, L.out_features,
                                                    L.in_features, w.gw[l], w.gb[l], w.slab[l])
                                    : wgrad_problem(t, w, dY, ld_dy, w.hid[l - 1], t.linear[l - 1].out_features,
                                                    L.out_features, L.in_features, w.gw[l], w.gb[l], w.slab[l]);
            if (l == 0) {
                p.x_idx = w.fidx;
                if (t.features_planes && !t.matmul_bf16) {
                    p.X3p = t.features_planes;
                    p.ld_x3 = t.feat_planes_ld;
                }
            }
            owner(L);
            wb.p[wb.count++] = p;
        }
    }
    if (dense) {
        tail.ad = dense->ad;
        tail.status = dense->status;
        wb.tail = &tail;
    }
    return launch_wgrad(wb, s, wg_events);
}
}  // namespace

// ---- eval-side setup the single-tower, eval-loss and autograd entries share -----------------
int stage_ids(const StageSeg* segs, int nsegs, uint32_t* status, const ttamm_tower* const* T, TowerWs* const* W,
              int ntowers, hipStream_t s) {
    int rc;
    StageArgs st;
    std::memset(&st, 0, sizeof(st));
    st.status = status;
    for (int i = 0; i < nsegs; ++i) st.seg[st.count++] = segs[i];
    if ((rc = launch_stage_rows(st, s))) return rc;
    // nn.Embedding(max_norm) renorms in eval mode too: the claim marks are cleared per call
    for (int k = 0; k < ntowers; ++k)
        if (W[k]->renorm_mark) {
            TTAMM_HIP(hipMemsetAsync(W[k]->renorm_mark, 0, (size_t)T[k]->id.rows * sizeof(int32_t), s));
            W[k]->renorm_tag = 1;
        }
    return TTAMM_OK;
}

int tower_forward_eval_mode(const ttamm_tower* const* T, TowerWs* const* W, int ntowers, int D, bool mimic,
                            hipStream_t s) {
    ttamm_tower te[2];
    const ttamm_tower* TT[2] = {nullptr, nullptr};
    TowerWs* WW[2] = {nullptr, nullptr};
    for (int k = 0; k < ntowers; ++k) {
        te[k] = *T[k];
        te[k].dropout = 0.f;
        TT[k] = &te[k];
        WW[k] = W[k];
    }
    ttamm_batch bt;
    std::memset(&bt, 0, sizeof(bt));
    return tower_forward(TT, WW, bt, D, mimic, s, ntowers);
}

}  // namespace ttamm

