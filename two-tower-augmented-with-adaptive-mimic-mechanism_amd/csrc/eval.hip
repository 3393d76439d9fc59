// The entries that run towers without the training step: the eval-mode single-tower forward,
// the validation-loss passes, and the training-mode tower forward / backward of the module-level
// autograd.  Each lays its towers out with plan_tower (tower.h) and sizes its workspace with a
// measuring pass over the same call.
#include <cstdint>
#include <cstring>

#include "tower.h"

namespace ttamm {

// ---- eval-mode tower forward (TowerEncoder.forward + augment) -----------------------------
namespace {
// Forward buffers; aug is the caller's `out`.  The gate and the concat projection go through
// t | a rows in the workspace (a when the tower has a mimic table); identity / sum fusion combine
// straight into aug.  No gate16 images: the gate runs on gate.hip or the generic path.
void plan_tower_eval(Arena& ar, const ttamm_tower& T, int64_t n, TowerWs& w) {
    TowerPlan o;
    o.io = uses_ef(T) ? IO_T : 0;
    o.mimic = T.mimic.weight != nullptr;
    o.claim_marks = true;
    plan_tower(ar, T, n, o, w);
}
}  // namespace

size_t tower_forward_workspace_size(const ttamm_tower& T, int64_t n) {
    Arena ar{nullptr, 0, 0, true};
    TowerWs w;
    plan_tower_eval(ar, T, n, w);
    return ar.off + 256;
}

int tower_forward_eval(const ttamm_tower& T, const int64_t* idx, const int64_t* fidx, int64_t n, int augment,
                       float* out, void* wsp, size_t ws_bytes, hipStream_t s) {
    const int D = out_dim(T);
    int rc;
    if ((rc = validate_tower(T, "tower", D, false))) return rc;
    if (augment && T.mimic.weight)
        TTAMM_REQUIRE(T.mimic.rows == T.id.rows && T.mimic.dim == D, "tower: mimic table shape does not match the tower");
    if (n <= 0) return TTAMM_OK;
    Arena ar{static_cast<char*>(wsp), ws_bytes, 0, false};
    TowerWs w;
    plan_tower_eval(ar, T, n, w);
    TTAMM_REQUIRE(ar.ok(), "workspace too small for tower forward");
    // ids outside the tables read row 0 (the Python mirror raises IndexError before calling);
    // nn.Embedding max_norm renorms in eval mode too (one lookup)
    const StageSeg seg{idx, w.idx_own, n, T.id.rows};
    const ttamm_tower* TT[1] = {&T};
    TowerWs* WW[1] = {&w};
    if ((rc = stage_ids(&seg, 1, nullptr, TT, WW, 1, s))) return rc;
    w.idx = w.idx_own;
    w.fidx = fidx == idx ? w.idx_own : fidx;
    w.aug = out;
    return tower_forward_eval_mode(TT, WW, 1, D, augment && T.mimic.weight, s);
}

// ---- validation loss: one forward-only batch of `_compute_loss` (training.py:854-910) --------
//   sample negatives (b.sample_negatives)          samplers.py:11-85, the step's Philox keying
//   stage + range-check users, [pos; neg]          bad ids set the status bit and read row 0
//   both towers, grouped, eval mode                dropout off, max_norm renorm kept
//                                                  (positives and negatives as two lookups)
//   scores + BCE terms, fixed-order mean           training.py:881-907
// Everything runs on the caller's stream.  The tables are read as they are: deferred AdamW
// tables (ttamm_table.last_step) must have been flushed (ttamm_flush_tables;
// FusedTrainStep.finish() does it).  No parameter or optimizer state is written, apart from the
// max_norm renorm of the looked-up ID rows.
namespace {
struct EvalWs {
    TowerWs user, item;
    float* partials = nullptr;
    int blocks = 0;
    float* ib_partials = nullptr;  // in-batch pass: inbatch_loss_kernel's block sums
    int ib_blocks = 0;
    InBatchLossArgs ib_lse{};      // in-batch softmax: the LSE pass (in_batch_loss)
};

// Forward buffers for B and B(1+N) rows, the staged ids, the weight pads / images the forward
// forms and the score partials: no backward buffer, gradient slab or coalesce scratch.  The
// in-batch pass adds its kernel's block partials (nothing B x B, no slab).
void plan_eval(Arena& ar, const ttamm_step_args& A, EvalWs& ws, bool in_batch = false) {
    const int64_t B = A.b.batch;
    const int N = A.b.num_neg;
    const int D = out_dim(A.user);
    TowerPlan o;
    o.io = IO_T | IO_AUG;
    o.mimic = A.mimic_enabled != 0;
    o.w16 = o.gw16 = o.claim_marks = true;
    ws.user.role = ROLE_USER;
    ws.item.role = ROLE_ITEM;
    plan_tower(ar, A.user, B, o, ws.user);
    plan_tower(ar, A.item, B * (1 + (int64_t)N), o, ws.item);
    ws.blocks = score_blocks(B, D);
    ws.partials = ar.take<float>((size_t)ws.blocks);
    if (in_batch && A.in_batch_loss == TTAMM_INBATCH_SOFTMAX) {  // the LSE pass's workspace
        ws.ib_lse.B = ws.ib_lse.Bc = B;
        float* w = ar.take<float>(inbatch_lse_floats(B, B));
        if (!ar.measuring) inbatch_lse_bind(ws.ib_lse, w);
    } else if (in_batch) {
        ws.ib_blocks = inbatch_loss_blocks(B, B);
        ws.ib_partials = ar.take<float>((size_t)ws.ib_blocks);
    }
}

int validate_eval(const ttamm_step_args& A, bool in_batch = false) {
    const int D = out_dim(A.user);
    int rc;
    if ((rc = validate_pair(A, false))) return rc;
    TTAMM_REQUIRE(A.phase == TTAMM_PHASE_ALL, "eval loss: phase must be 0, the whole batch in one call (no sharded validation pass)");
    if (in_batch) {  // ttamm_eval_loss_inbatch: the in_batch field is not consulted, N = 0 is legal
        TTAMM_REQUIRE(A.b.num_neg >= 0 && A.b.num_neg <= 64,
                      "eval loss (in-batch): b.num_neg (negatives_per_positive) must be in [0, 64]");
        if ((rc = inbatch_loss_check(D))) return rc;
        TTAMM_REQUIRE(A.in_batch_loss == TTAMM_INBATCH_BCE || A.in_batch_loss == TTAMM_INBATCH_SOFTMAX,
                      "in_batch_loss must be 0 (the BCE mean) or 1 (the softmax cross-entropy)");
        if (A.in_batch_loss == TTAMM_INBATCH_SOFTMAX) {
            TTAMM_REQUIRE(A.b.num_neg == 0,
                          "in_batch_loss: the softmax objective needs b.num_neg == 0 (sampled negatives do not join "
                          "the denominator)");
            if ((rc = inbatch_softmax_check(A.in_batch_inv_temperature))) return rc;
        }
    } else {
        TTAMM_REQUIRE(A.in_batch == 0, "eval loss: in_batch must be 0 (_compute_loss scores sampled negatives only)");
        if ((rc = score_eval_check(A.b.num_neg, D))) return rc;
    }
    TTAMM_REQUIRE(A.b.batch > 0, "empty batch");
    return validate_mimic_pair(A);
}
}  // namespace

size_t eval_loss_workspace_size(const ttamm_step_args& A) {
    Arena ar{nullptr, 0, 0, true};
    EvalWs ws;
    plan_eval(ar, A, ws);
    return ar.off + 256;
}

size_t eval_loss_inbatch_workspace_size(const ttamm_step_args& A) {
    if (A.b.batch <= 0 || A.b.num_neg < 0) return 0;
    Arena ar{nullptr, 0, 0, true};
    EvalWs ws;
    plan_eval(ar, A, ws, true);
    return ar.off + 256;
}

// in_batch: ttamm_eval_loss_inbatch — the positives' logits come from S = U P^T
// (inbatch_loss_kernel on U.aug and I.aug rows [0, B)), the scorer adds the sampled negatives'
// terms only (none with N == 0) and one finalize divides by B (B + N).
static int eval_loss_run(const ttamm_step_args& A, float* logits_out, bool in_batch, hipStream_t s) {
    int rc;
    if ((rc = validate_eval(A, in_batch))) return rc;
    TTAMM_REQUIRE(A.loss_out && A.status && A.workspace, "eval loss: loss_out, status and workspace are required");
    TTAMM_REQUIRE(A.b.users && A.b.pos_items, "eval loss: b.users / b.pos_items missing");
    const int D = out_dim(A.user);
    const bool mimic = A.mimic_enabled != 0;
    const int64_t B = A.b.batch;
    const int N = A.b.num_neg;
    EvalWs ws;
    Arena ar{static_cast<char*>(A.workspace), A.workspace_bytes, 0, false};
    plan_eval(ar, A, ws, in_batch);
    TTAMM_REQUIRE(ar.ok(), "workspace too small for this eval loss batch");
    TowerWs &U = ws.user, &I = ws.item;
    int64_t* neg_rows = I.idx_own + B;
    const int64_t* neg_src = A.b.neg_items;
    if (A.b.sample_negatives && N > 0) {  // the training step's draws for (seed, counter, row_base)
        const int64_t num_items = A.num_items_global > 0 ? A.num_items_global : A.item.id.rows;
        int64_t* dst = A.b.neg_items ? A.b.neg_items : neg_rows;
        if ((rc = launch_sample_negatives(A.b.users, B, N, num_items, A.b.pos_offsets, A.b.pos_values, A.user.id.rows,
                                          A.b.seed, A.b.counter, A.row_base * N, dst, nullptr, A.status, s)))
            return rc;
        neg_src = dst;
    }
    TTAMM_REQUIRE(N == 0 || neg_src != nullptr, "negatives must be given when sample_negatives == 0");
    const StageSeg segs[3] = {{A.b.users, U.idx_own, B, A.user.id.rows},
                              {A.b.pos_items, I.idx_own, B, A.item.id.rows},
                              {neg_src, neg_rows, B * N, A.item.id.rows}};
    const ttamm_tower* TT[2] = {&A.user, &A.item};
    TowerWs* WW[2] = {&U, &I};
    if ((rc = stage_ids(segs, N > 0 ? 3 : 2, A.status, TT, WW, 2, s))) return rc;
    U.idx = U.fidx = U.idx_own;
    I.idx = I.fidx = I.idx_own;
    // max_norm: the users are one lookup, the positives and the negatives the item table's two
    // (training.py:875,887)
    I.renorm_split = B;
    if ((rc = tower_forward_eval_mode(TT, WW, 2, D, mimic, s))) return rc;
    EvalScoreArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.B = B;
    sa.N = N;
    sa.D = D;
    sa.user_aug = U.aug;
    sa.item_aug = I.aug;
    sa.ld_item = D;
    sa.partials = ws.partials;
    sa.blocks = ws.blocks;
    sa.logits = logits_out;
    const InBatchProblem ibp = {U.aug, D, B, I.aug, D, B, D, 0};  // S = U P^T over the batch's own positives
    if (in_batch && A.in_batch_loss == TTAMM_INBATCH_SOFTMAX) {  // one LSE pass, the mean of its B terms
        InBatchLossArgs& l = ws.ib_lse;
        static_cast<InBatchProblem&>(l) = ibp;
        if ((rc = launch_inbatch_lse(l, A.in_batch_inv_temperature, s))) return rc;
        return launch_eval_loss_inbatch_finalize(nullptr, 0, l.loss_part, inbatch_lse_parts(B), B, B, A.loss_out,
                                                 A.loss_accum, A.status, s);
    }
    if (in_batch) {
        InBatchLossArgs ib{};
        static_cast<InBatchProblem&>(ib) = ibp;
        ib.loss_part = ws.ib_partials;
        if ((rc = launch_inbatch_loss(ib, s))) return rc;
        sa.skip_pos = 1;
        sa.logits = nullptr;  // S is never stored
        if (N > 0 && (rc = launch_score_eval(sa, s))) return rc;
        return launch_eval_loss_inbatch_finalize(ws.partials, N > 0 ? ws.blocks : 0, ws.ib_partials, ws.ib_blocks,
                                                 B * (B + (int64_t)N), B, A.loss_out, A.loss_accum, A.status, s);
    }
    if ((rc = launch_score_eval(sa, s))) return rc;
    return launch_eval_loss_finalize(ws.partials, ws.blocks, B * (1 + (int64_t)N), B, A.loss_out, A.loss_accum, A.status, s);
}

int eval_loss(const ttamm_step_args& A, float* logits_out, hipStream_t s) { return eval_loss_run(A, logits_out, false, s); }

int eval_loss_inbatch(const ttamm_step_args& A, hipStream_t s) { return eval_loss_run(A, nullptr, true, s); }


// ---- training-mode tower forward / backward (module-level autograd) ------------------------
// TowerEncoder.forward under autograd (encoders.py:221-255) in two calls: the forward keeps its
// activations in the workspace, the backward (same tower, rows and workspace) runs the tower's
// backward kernels — gate, dgrad chain, one grouped weight-gradient launch — into the caller's
// gradient arena (tower_grad_floats: per Linear weight then bias, 256-B aligned pieces) and
// writes the ID rows' gradient per position (and, identity feature encoder, the feature rows').
namespace {
void plan_tower_train(Arena& ar, const ttamm_tower& T, int64_t n, TowerWs& w) {
    WgradShape shapes[TTAMM_MAX_LINEAR + 2];
    const int ns = wgrad_shapes(T, n, shapes);
    int rps[kWgradClasses] = {512, 512, 512, 512};
    if (ns) wgrad_rows_per_split(shapes, ns, rps);
    for (int c = 0; c < kWgradClasses; ++c) w.wgrad_rps[c] = rps[c];
    // t and dT are the caller's out / d_out; no mimic rows, no aug
    TowerPlan o;
    o.backward = true;
    o.gw16 = o.claim_marks = o.f_any = true;
    w.role = ROLE_USER;
    plan_tower(ar, T, n, o, w);
}

int bind_tower_train(const ttamm_tower& T, const int64_t* idx, const int64_t* fidx, int64_t n, void* wsp,
                     size_t ws_bytes, TowerWs& w) {
    Arena ar{static_cast<char*>(wsp), ws_bytes, 0, false};
    plan_tower_train(ar, T, n, w);
    TTAMM_REQUIRE(ar.ok(), "workspace too small for the training tower forward / backward");
    w.idx = w.idx_own;
    w.fidx = fidx == idx ? w.idx_own : fidx;  // caller-gathered feature rows: fidx = null (row r)
    w.key_split = n;
    return TTAMM_OK;
}
}  // namespace

size_t tower_grad_floats_of(const ttamm_tower& T) { return tower_grad_floats(T); }

size_t tower_train_workspace_size(const ttamm_tower& T, int64_t n) {
    Arena ar{nullptr, 0, 0, true};
    TowerWs w;
    plan_tower_train(ar, T, n, w);
    return ar.off + 256;
}

int tower_train_forward(const ttamm_tower& T, const int64_t* idx, const int64_t* fidx, int64_t n,
                        const uint8_t* const* keep_masks, uint64_t seed, uint64_t counter, float* out, void* wsp,
                        size_t ws_bytes, hipStream_t s) {
    const int D = out_dim(T);
    int rc;
    if ((rc = validate_tower(T, "tower", D, false))) return rc;
    if (n <= 0) return TTAMM_OK;
    TowerWs w;
    if ((rc = bind_tower_train(T, idx, fidx, n, wsp, ws_bytes, w))) return rc;
    const ttamm_tower* TT[2] = {&T, nullptr};
    TowerWs* WW[2] = {&w, nullptr};
    // ids outside the table read row 0 (the Python mirror raises IndexError before calling)
    const StageSeg seg{idx, w.idx_own, n, T.id.rows};
    if ((rc = stage_ids(&seg, 1, nullptr, TT, WW, 1, s))) return rc;
    w.t = out;
    w.t_ld = D;
    ttamm_batch bt;
    std::memset(&bt, 0, sizeof(bt));
    bt.seed = seed;
    bt.counter = counter;
    for (int l = 0; keep_masks && l + 1 < T.n_linear; ++l) bt.user_keep_mask[l] = keep_masks[l];
    return tower_forward(TT, WW, bt, D, false, s, 1);
}

int tower_train_backward(const ttamm_tower& T, const int64_t* idx, const int64_t* fidx, int64_t n,
                         const uint8_t* const* keep_masks, const float* d_out, float* grad_arena, float* d_id_rows,
                         float* d_feat_rows, void* wsp, size_t ws_bytes, hipStream_t s) {
    const int D = out_dim(T);
    const int Did = T.id.dim;
    int rc;
    if ((rc = validate_tower(T, "tower", D, false))) return rc;
    const size_t ng = tower_grad_floats(T);
    if (n <= 0) {
        if (ng) TTAMM_HIP(hipMemsetAsync(grad_arena, 0, ng * sizeof(float), s));
        return TTAMM_OK;
    }
    TTAMM_REQUIRE(d_out && (ng == 0 || grad_arena), "tower backward: d_out / grad_arena missing");
    TowerWs w;
    if ((rc = bind_tower_train(T, idx, fidx, n, wsp, ws_bytes, w))) return rc;
    w.dT = d_out;
    w.dT_ld = D;
    float* cur = grad_arena;
    carve_grads(T, w, cur);
    // non-ReLU layers read the forward's keep bytes: the injected masks again, or the ones the
    // forward drew into the workspace
    for (int l = 0; l + 1 < T.n_linear; ++l) w.keep[l] = keep_masks && keep_masks[l] ? keep_masks[l] : w.mask[l];
    const ttamm_tower* TT[2] = {&T, nullptr};
    TowerWs* WW[2] = {&w, nullptr};
    if (T.fusion != TTAMM_FUSION_IDENTITY)
        if ((rc = tower_backward(TT, WW, D, s, 1))) return rc;
    // d(ID rows): [e | f] towers take dEF[:, :Did]; sum / identity fusion pass dT to e
    const float* de = uses_ef(T) ? w.dEF : d_out;
    const int64_t ld_de = uses_ef(T) ? efw(T) : D;
    if (d_id_rows && (rc = launch_add_rows(de, ld_de, nullptr, 0, n, Did, d_id_rows, Did, s))) return rc;
    if (d_feat_rows) {  // identity feature encoder: f = the feature row, its gradient is dEF[:, Did:] / dT
        TTAMM_REQUIRE(T.n_linear == 0 && T.fusion != TTAMM_FUSION_IDENTITY,
                      "tower backward: feature-row gradients exist for the identity feature encoder only");
        const float* df = uses_ef(T) ? w.dEF + Did : d_out;
        const int fo = fo_dim(T);
        if ((rc = launch_add_rows(df, ld_de, nullptr, 0, n, fo, d_feat_rows, fo, s))) return rc;
    }
    return TTAMM_OK;
}


}  // namespace ttamm
