// One tower (TowerEncoder, encoders.py:221-255) on the device: its workspace, the one planner
// that lays the workspace out, and its forward / backward drivers (tower.hip).  Internal to the
// library: the training step (step.hip) and the eval / autograd entries (eval.hip) share it.
#pragma once
#include <cstdint>

#include "kernels.h"

namespace ttamm {

enum Role { ROLE_USER = 0, ROLE_ITEM = 1 };

struct TowerWs {
    int role = ROLE_USER;
    int64_t R = 0;
    const int64_t* idx = nullptr;   // ID / mimic table rows
    const int64_t* fidx = nullptr;  // feature rows (null: row r)
    int64_t* idx_own = nullptr;     // staged (range-checked) rows: users / 1-process items [pos; neg] /
                                    // sharded owner's requested local item rows
    // dropout stream key of row r (see GemmProblem::row_key)
    const int64_t* row_key = nullptr;
    int64_t key_base0 = 0, key_base1 = 0, key_split = 0;
    // ID-table max_norm: per-row claim marks (persistent, zero once) and this call's tag base
    int32_t* renorm_mark = nullptr;
    int32_t renorm_tag = 0;
    int64_t renorm_split = 0;  // item tower: positives [0, split) are one lookup, negatives the next
    int64_t renorm_key_split = 0;  // sharded owner: requests with row_key < this (positives) are one lookup
    float* hid[TTAMM_MAX_LINEAR] = {};
    float* dhid[TTAMM_MAX_LINEAR] = {};
    // non-ReLU activations: each hidden layer's pre-activation, its drawn keep bytes (dropout
    // without an injected mask), and the keep bytes the backward reads (injected or drawn)
    float* pre[TTAMM_MAX_LINEAR] = {};
    uint8_t* mask[TTAMM_MAX_LINEAR] = {};
    const uint8_t* keep[TTAMM_MAX_LINEAR] = {};
    float* ef = nullptr;    // gated: [R, 2D] = [e | f]
    float* e = nullptr;     // non-gated: [R, D]
    float* f = nullptr;     // sum fusion: [R, D]
    float* z = nullptr;     // gate hidden [R, Hg]
    float* dz = nullptr;
    float* g = nullptr;
    float* t = nullptr;     // [R, t_ld] (a alongside at the same stride)
    float* a = nullptr;
    int64_t t_ld = 0;
    float* aug = nullptr;   // [R, D] or null (sharded item owner)
    const float* dT = nullptr;  // [R, dT_ld]
    float* dT_own = nullptr;
    int64_t dT_ld = 0;
    const float* dA = nullptr;  // mimic-table grad rows (user: all rows; item: positives or all)
    float* dA_own = nullptr;
    int64_t dA_ld = 0;
    int64_t dA_split = 0;       // rows < dA_split read dA, the rest read dT
    const int64_t* xu = nullptr;  // sharded owner, compact exchange rows: row units (GateTower::xu)
    float* dq = nullptr;
    float* dEF = nullptr;  // [R, 2D]
    float* gw[TTAMM_MAX_LINEAR] = {};
    float* gb[TTAMM_MAX_LINEAR] = {};
    float* ggw[2] = {};
    float* ggb[2] = {};
    float* slab[TTAMM_MAX_LINEAR + 2] = {};
    CoalesceWs co{};
    CatchupList cl{};  // deferred AdamW: the batch's rows to bring current, grouped by lag
    float* side_id = nullptr;
    float* side_mimic = nullptr;
    float* piece_e = nullptr;
    float* piece_a = nullptr;
    float* wpad = nullptr;  // first feature layer weight, in_features padded to a multiple of 4
    uint16_t* w16 = nullptr;  // bf16 towers with bf16 feature rows: the weight rounded, padded to % 8
    uint16_t* gw16 = nullptr;  // bf16 gated towers (D == Hg in {128, 256}): the fused gate's weight images
    bool gw16_ready = false;   // formed by this call's forward (the weights do not change before its backward)
    int wgrad_rps[kWgradClasses] = {512, 512, 512, 512};  // split-K rows of the weight gradients, per tile class
};

inline int round4(int x) { return (x + 3) / 4 * 4; }
inline int round8(int x) { return (x + 7) / 8 * 8; }
// the first feature layer's forward on bf16 operands in memory (ttamm_tower.features_bf16)
inline bool uses_w16(const ttamm_tower& T) {
    return T.matmul_bf16 && T.features_bf16 != nullptr && T.fusion != TTAMM_FUSION_IDENTITY && T.n_linear > 0;
}
// gated and concat towers keep [e | f] rows (the gate's / projection's input) and their gradient
inline bool uses_ef(const ttamm_tower& T) { return T.fusion == TTAMM_FUSION_GATED || T.fusion == TTAMM_FUSION_CONCAT; }
// Linear layers after the feature encoder: the gate's two, or the concat projection
inline int fusion_linears(const ttamm_tower& T) {
    return T.fusion == TTAMM_FUSION_GATED ? 2 : T.fusion == TTAMM_FUSION_CONCAT ? 1 : 0;
}
// widths of a tower: the ID rows (Did), the feature encoder's output (Fo), the [e | f] rows of
// gated / concat fusion (Did + Fo) and the tower output (concat: the projection's output_dim,
// encoders.py:211-217; otherwise Did).  Everything downstream of the tower (scores, mimic
// tables, the exchange rows) is output-wide; only concat lets the output differ from Did.
inline int fo_dim(const ttamm_tower& T) { return T.n_linear ? T.linear[T.n_linear - 1].out_features : T.feat_dim; }
inline int efw(const ttamm_tower& T) { return T.id.dim + fo_dim(T); }
inline int out_dim(const ttamm_tower& T) { return T.fusion == TTAMM_FUSION_CONCAT ? T.gate[0].out_features : T.id.dim; }
inline bool needs_wpad(const ttamm_tower& T) {
    return T.fusion != TTAMM_FUSION_IDENTITY && T.n_linear > 0 && T.linear[0].in_features % 4 != 0;
}

// Validate one tower against the reference's own constraints.
int validate_tower(const ttamm_tower& T, const char* name, int D, bool training);
// both towers, then what the user / item pair must share: output width and matmul precision
int validate_pair(const ttamm_step_args& A, bool training);
// mimic_enabled: both mimic tables present and shaped like their tower
int validate_mimic_pair(const ttamm_step_args& A);

// What one call needs of a tower's workspace (plan_tower).  The optional weight copies select
// kernels, not only sizes: gate_group reads w.gw16, the first feature layer w.w16 / w.wpad.
enum { IO_T = 1, IO_AUG = 2, IO_DT = 4, IO_ALL = 7 };  // t | a, aug, dT | dA rows
struct TowerPlan {
    bool backward = false;  // dhid, pre, mask, dEF, dz, dq and the split-K slabs (w.wgrad_rps chosen before)
    int io = 0;             // IO_*: the rows that live in the workspace; the others are the caller's to bind
    bool mimic = false;     // the mimic rows exist: a (with t) and dA (with dT)
    int64_t dA_rows = 0;    // rows of dA (TowerWs::dA_split)
    bool w16 = false;       // the bf16 first-layer weight when uses_w16 (ttamm_tower.features_bf16 honoured)
    bool gw16 = false;      // the fused gate's weight images when gate16_supported
    bool claim_marks = false;  // max_norm claim marks, cleared per call (the step's sit in its scratch head)
    bool f_any = false;     // f for identity fusion too, not for sum alone
};
// The one layout of a tower's buffers over R rows: staged ids, activations, their gradients, the
// weight copies.  Every entry sizes with a measuring Arena pass over the call its run makes.
void plan_tower(Arena& ar, const ttamm_tower& T, int64_t R, const TowerPlan& o, TowerWs& w);

size_t tower_grad_floats(const ttamm_tower& T);
void carve_grads(const ttamm_tower& T, TowerWs& w, float*& cur);
int wgrad_shapes(const ttamm_tower& T, int64_t R, WgradShape* out);

bool gate_choice(const ttamm_tower* const* T, const bool* has16, int ntowers, int D, int& hg, int& planes);

// part FWD_GATHER: ID-row renorm + gather; FWD_FEAT: feature encoder; FWD_FUSION: gate / combine
// (reads the mimic rows)
enum { FWD_GATHER = 1, FWD_FUSION = 2, FWD_FEAT = 4, FWD_MLP = FWD_GATHER | FWD_FEAT, FWD_ALL = 7 };
int tower_forward(const ttamm_tower* T[2], TowerWs* W[2], const ttamm_batch& bt, int D, bool mimic, hipStream_t s,
                  int ntowers, void* const* l0_events = nullptr, int part = FWD_ALL, hipEvent_t after_l0 = nullptr);
// wg_events (optional, 2 events): around the wide weight-gradient GEMM launch (bench)
// part BWD_GATE: the fusion's backward (dEF, the ID rows' gradient with it); BWD_MLP: the feature
// MLP's dgrad chain and every weight gradient
enum { BWD_GATE = 1, BWD_MLP = 2, BWD_ALL = 3 };
// dense (optional; the one-process step without clipping): the AdamW update of every Linear
// follows its weight gradient's slab reduce in the same kernel (kernels.h WgradTail), so the
// caller launches no dense update
struct DenseTail {
    AdamConsts ad;
    const uint32_t* status;
};
int tower_backward(const ttamm_tower* T[2], TowerWs* W[2], int D, hipStream_t s, int ntowers,
                   void* const* wg_events = nullptr, int part = BWD_ALL, const DenseTail* dense = nullptr);

// Stage and range-check id segments (ids outside a table read row 0 and, with a status word, set
// its bit), then clear and tag the claim marks of the towers that have max_norm.
int stage_ids(const StageSeg* segs, int nsegs, uint32_t* status, const ttamm_tower* const* T, TowerWs* const* W,
              int ntowers, hipStream_t s);
// tower_forward on eval-mode copies of the towers: dropout off, a zero ttamm_batch (the caller's
// descriptors are not changed)
int tower_forward_eval_mode(const ttamm_tower* const* T, TowerWs* const* W, int ntowers, int D, bool mimic,
                            hipStream_t s);

}  // namespace ttamm
