// Native executor of one training step (the body of `_train_one_epoch`,
// training.py:726-831), issued as a fixed sequence of gfx950 kernels on one HIP stream.
//
//   sample negatives                      samplers.py:11-85                (a11)
//   tower forward (user & item grouped)   encoders.py:221-255              (a1, a3, a4)
//     hidden Linear+ReLU+Dropout GEMMs    gathered feature rows, MFMA fp32
//     final Linear -> f ; ID gather -> e  into one [rows, 2D] "ef" buffer
//     gate GEMM 1 (ReLU), gate GEMM 2 (sigmoid, mix, mimic augment)      adaptive_mimic.py:88-95 (a2)
//   score + BCE + mimic MSE fwd/bwd       training.py:770-803              (a5-a7)
//   tower backward (dgrad chain grouped, then all weight grads in one launch)
//   coalesce row grads, SparseAdam (ID tables), AdamW touched rows        (a9, a5)
//   AdamW(g=0) stream over the full mimic tables, side-row scatter         (a5, a10)
//   AdamW on the MLP / gate weights                                        (a10)
//
// A row-sharded multi-GPU step runs the same pieces as phases (ttamm.h TTAMM_PHASE_*): the
// item tower of a rank runs over the item rows it owns, for whoever requested them; the
// host moves (t | a) and (dT | dA) rows between phases and all-reduces the gradient arena.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tower.h"

namespace ttamm {

namespace {

struct StepWs {
    TowerWs user, item;
    float* partials = nullptr;
    uint32_t* prologue_done = nullptr;  // completion counter of step_prologue_kernel (zero between calls)
    int64_t* keys_own = nullptr;        // sharded owner: staged request keys [item_rows_capacity]
    // compact exchange rows (ttamm_step_args.exchange_counts): the first unit of each owned row
    // (~unit for a negative), formed with the ITEM_FWD staging
    int64_t* own_units = nullptr;
    int score_blocks = 0;
    // in-batch negatives (ttamm_step_args.in_batch)
    bool ib_on = false;
    InBatchArgs ib{};
    float* ib_du = nullptr;   // [B, D]
    float* ib_dp = nullptr;   // [B, D] (one process; sharded: the caller's inbatch_dp)
    int ib_parts = 0;
    // softmax objective (ttamm_step_args.in_batch_loss): the LSE pass, which owns the loss
    bool ib_softmax = false;
    InBatchLossArgs ib_lse{};
    bool cal_on = false;  // category-alignment loss this step
    CalArgs cal{};
    // gradient clipping (ttamm_hparams.grad_clip_norm)
    bool clip_on = false;
    float* clip_partials = nullptr;
    int clip_parts = 0;
    float* clip_coef = nullptr;
};

// The category-alignment loss runs when categories are given and its weight is positive
// (training.py:805: `if lambda_cal > 0`; _category_alignment_loss returns 0 without them).
bool cal_enabled(const ttamm_step_args& A) {
    return A.item_categories != nullptr && A.hp.lambda_category_alignment > 0.0;
}

bool sharded(const ttamm_step_args& A) { return A.phase != TTAMM_PHASE_ALL; }
// compact exchange rows (ttamm.h ttamm_step_args.exchange_counts)
bool compact_exchange(const ttamm_step_args& A) { return sharded(A) && A.exchange_counts != nullptr; }
int64_t global_batch(const ttamm_step_args& A) { return A.global_batch > 0 ? A.global_batch : A.b.batch; }
// the in-batch objective is the softmax cross-entropy over the rows of S (ttamm.h in_batch_loss)
bool softmax_loss(const ttamm_step_args& A) { return A.in_batch_loss == TTAMM_INBATCH_SOFTMAX; }

// Workspace layout.  Deterministic in the arguments, so every phase call of a sharded step
// finds the previous phases' activations where it left them.
// Per-row scratch of the row grouping (CoalesceWs cnt / first / fill) comes first in the
// workspace: its offsets depend only on the table sizes, so it stays in place (and zero between
// calls, as launch_coalesce leaves it) whatever the batch size.  The caller zeroes the
// workspace once.
void plan_scratch(Arena& ar, const ttamm_step_args& A, StepWs& ws) {
    coalesce_bind_scratch(ws.user.co, ar.take<int32_t>(coalesce_scratch_ints(A.user.id.rows)), A.user.id.rows);
    coalesce_bind_scratch(ws.item.co, ar.take<int32_t>(coalesce_scratch_ints(A.item.id.rows)), A.item.id.rows);
    if (cal_enabled(A)) {
        const int64_t ncat = std::min<int64_t>(A.num_categories, 65535);
        coalesce_bind_scratch(ws.cal.co, ar.take<int32_t>(coalesce_scratch_ints(ncat)), ncat);
    }
    if (A.user.id.max_norm > 0.0) ws.user.renorm_mark = ar.take<int32_t>(A.user.id.rows);
    if (A.item.id.max_norm > 0.0) ws.item.renorm_mark = ar.take<int32_t>(A.item.id.rows);
    // step_prologue_kernel's completion counter: its last block resets it, so it must sit at a
    // batch-size-independent offset (a short last batch must find it zero, not old activations)
    ws.prologue_done = ar.take<uint32_t>(1);
}

void plan_coalesce(Arena& ar, CoalesceWs& co, int64_t R) {
    co.keys_out = ar.take<int32_t>(R);
    co.vals_out = ar.take<int32_t>(R);
    co.vals_tmp = ar.take<int32_t>(R);
    co.lead = ar.take<int32_t>(R);
    // lead_cnt / seglong double as the segment scan's tile totals: ceil(entries / 256) of them
    co.lead_cnt = ar.take<int32_t>(std::max<int64_t>(R, 257));
    co.seglong = ar.take<int32_t>(std::max<int64_t>(R, 257));
    co.seg_start = ar.take<int32_t>(R + 1);
    co.n_unique = ar.take<int32_t>(1);
}

int plan(Arena& ar, const ttamm_step_args& A, StepWs& ws) {
    const int64_t B = A.b.batch;
    const int N = A.b.num_neg;
    const int D = out_dim(A.user);
    const bool mimic = A.mimic_enabled != 0;
    const bool shard = sharded(A);
    plan_scratch(ar, A, ws);
    {
        WgradShape shapes[2 * (TTAMM_MAX_LINEAR + 2)];
        int n = wgrad_shapes(A.user, B, shapes);
        n += wgrad_shapes(A.item, shard ? A.item_rows_capacity : B * (1 + N), shapes + n);
        int rps[kWgradClasses];
        wgrad_rows_per_split(shapes, n, rps);
        for (int c = 0; c < kWgradClasses; ++c) ws.user.wgrad_rps[c] = ws.item.wgrad_rps[c] = rps[c];
    }
    // ext_io: the item tower's t / a / dT / dA live in the caller's exchange buffers
    auto tower = [&](const ttamm_tower& T, TowerWs& w, int64_t R, bool ext_io, int64_t dA_rows) {
        TowerPlan o;
        o.backward = true;
        o.io = ext_io ? 0 : IO_ALL;
        o.mimic = mimic;
        o.dA_rows = dA_rows;
        o.w16 = o.gw16 = true;
        plan_tower(ar, T, R, o, w);  // the claim marks are plan_scratch's
        plan_coalesce(ar, w.co, R);
        if (A.adam_history && A.history_capacity > 1) {
            const int cap = A.history_capacity;
            catchup_bind(w.cl, ar.take<int32_t>(catchup_list_ints(R, cap)), R, cap);
        }
        w.piece_e = ar.take<float>((size_t)R * T.id.dim);
        if (mimic) w.piece_a = ar.take<float>((size_t)R * D);
        if (T.id.optimizer == TTAMM_OPT_DENSE) w.side_id = ar.take<float>((size_t)R * 3 * T.id.dim);
        if (mimic) w.side_mimic = ar.take<float>((size_t)R * 3 * D);
    };
    ws.user.role = ROLE_USER;
    ws.item.role = ROLE_ITEM;
    tower(A.user, ws.user, B, false, B);
    if (shard) {
        tower(A.item, ws.item, A.item_rows_capacity, true, 0);
        ws.keys_own = ar.take<int64_t>(A.item_rows_capacity);
        ws.own_units = ar.take<int64_t>(A.item_rows_capacity);
    }
    else
        tower(A.item, ws.item, B * (1 + N), false, B);
    ws.score_blocks = score_blocks(B, D);
    ws.partials = ar.take<float>((size_t)ws.score_blocks * 3);
    if (A.hp.grad_clip_norm > 0.0) {
        ws.clip_on = true;
        // [tables' total (sharded: all-reduced)] + both towers' row partials + the dense partials
        ws.clip_parts = 1 + rows_sumsq_blocks(B, A.user.id.dim) +
                        rows_sumsq_blocks(shard ? A.item_rows_capacity : B * (1 + N), A.item.id.dim) +
                        kDenseSumsqBlocks;
        ws.clip_partials = ar.take<float>((size_t)ws.clip_parts);
        ws.clip_coef = ar.take<float>(1);
    }
    if (A.in_batch) {
        ws.ib_on = true;
        const int64_t Bc = shard ? global_batch(A) : B;
        size_t su, sp, parts;
        inbatch_workspace_floats(B, Bc, D, &su, &sp, &parts);
        ws.ib.slab_u = ar.take<float>(su);
        ws.ib.slab_p = ar.take<float>(sp);
        ws.ib.loss_part = ar.take<float>(parts);
        ws.ib_parts = (int)parts;
        ws.ib_du = ar.take<float>((size_t)B * D);
        if (!shard) ws.ib_dp = ar.take<float>((size_t)B * D);
        if (softmax_loss(A)) {
            ws.ib_softmax = true;
            ws.ib_lse.B = B, ws.ib_lse.Bc = Bc;
            float* w = ar.take<float>(inbatch_lse_floats(B, Bc));
            if (!ar.measuring) inbatch_lse_bind(ws.ib_lse, w);
        }
    }
    if (cal_enabled(A)) {
        // one process: the batch's item rows; sharded: this requester's rows, with the per-category
        // sums and scatters in the caller's all-reduce buffers (slot space = category ids)
        CalArgs& c = ws.cal;
        ws.cal_on = true;
        const int64_t R = B * (1 + N);
        c.R = R;
        c.D = D;
        c.nseg_max = (int)std::min<int64_t>(R, std::max<int64_t>(1, std::min<int64_t>(A.num_categories, 65535)));
        const int64_t slots = shard ? A.num_categories : c.nseg_max;
        const int pieces = cal_max_pieces(R, c.nseg_max);
        c.catrow = ar.take<int64_t>(R);
        plan_coalesce(ar, c.co, R);
        c.co.sorted = 1;  // categories ascending, as the reference's loop (training.py:567)
        c.pcount = ar.take<int32_t>(c.nseg_max);
        c.pstart = ar.take<int32_t>(c.nseg_max);
        c.psum = ar.take<float>((size_t)pieces * D);
        c.mean = ar.take<float>((size_t)c.nseg_max * D);
        c.pslab = ar.take<float>((size_t)pieces * D * D);
        if (shard) {
            c.gstats = A.cal_stats;
            c.cov = A.cal_scatter;
        } else {
            c.cov = ar.take<float>((size_t)c.nseg_max * D * D);
        }
        c.part = ar.take<float>(slots);
        c.flag = ar.take<int32_t>(slots);
        c.gmajor = ar.take<float>((size_t)D * D);
        c.out = ar.take<float>(2);
    }
    // gradient arena: the caller's all-reduce buffer when sharded, else workspace
    float* arena = shard ? A.dense_grads : ar.take<float>(tower_grad_floats(A.user) + tower_grad_floats(A.item));
    carve_grads(A.user, ws.user, arena);
    carve_grads(A.item, ws.item, arena);
    return TTAMM_OK;
}

// Deferred exact AdamW(g = 0) (ttamm.h ttamm_table.last_step).
struct Deferred {
    bool on = false;
    AdamConsts* hist = nullptr;
    int cap = 0;
    int slices = 1;
    int32_t step = 0;  // the dense step this call executes
    int decoupled = 1;
    int fast = 0;  // TTAMM_G0_FAST arithmetic for the g = 0 updates
    int sgd = 0;   // torch.optim.SGD dense group: the g = 0 replay is sgd_elem's (replay_sgd_kernel)
    const uint32_t* status = nullptr;  // poisoned: the step writes nothing
};

// The part of a replay launch that the optimizer fixes; the caller adds the row segments.
ReplayArgs replay_header(const Deferred& df, int32_t target, int stamp) {
    ReplayArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.hist = df.hist;
    ra.cap = df.cap;
    ra.decoupled = df.decoupled;
    ra.sgd = df.sgd;
    ra.fast_g0 = df.fast;
    ra.status = df.status;
    ra.target = target;
    ra.stamp = stamp;
    return ra;
}

// The tables of a tower that belong to the dense (AdamW) group.
int dense_tables(const ttamm_tower& t, bool mimic, const ttamm_table* out[2]) {
    int n = 0;
    if (mimic) out[n++] = &t.mimic;
    if (t.id.optimizer == TTAMM_OPT_DENSE) out[n++] = &t.id;
    return n;
}

ReplaySeg replay_seg(const ttamm_table& tb) {
    ReplaySeg g;
    std::memset(&g, 0, sizeof(g));
    g.p = tb.weight;
    g.m = tb.exp_avg;
    g.v = tb.exp_avg_sq;
    g.last = tb.last_step;
    g.touched = tb.touched;
    g.dim = tb.dim;
    return g;
}

// The rolling slice of the deferred AdamW(g = 0): this step's 1/slices of every dense-group
// table's rows brought to `target` (every row's lag stays below the history ring).
int replay_slice(const ttamm_tower* const* T, int n, bool mimic, const Deferred& df, int32_t target, int stamp,
                 void* const* events, hipStream_t s) {
    ReplayArgs ra = replay_header(df, target, stamp);
    const int slice = (int)(((int64_t)target % df.slices + df.slices) % df.slices);
    for (int k = 0; k < n; ++k) {
        const ttamm_table* tabs[2];
        const int nt = dense_tables(*T[k], mimic, tabs);
        for (int i = 0; i < nt; ++i) {
            ReplaySeg g = replay_seg(*tabs[i]);
            const int64_t per = (tabs[i]->rows + df.slices - 1) / df.slices;
            g.row_lo = std::min<int64_t>(tabs[i]->rows, slice * per);
            g.row_hi = std::min<int64_t>(tabs[i]->rows, g.row_lo + per);
            ra.seg[ra.count++] = g;
        }
    }
    return launch_replay(ra, s, events);
}

// Before a tower reads its rows (part A): count the batch's rows — which marks each row's first
// position — and, deferred, bring the dense-group rows it touches current to step - 1 (each row
// once): the rows behind, listed by lag (the list build stamps them current — a replay that runs
// before this step's row updates, the aux stream's slice or a flush after a poisoned step, must
// see them current to step - 1), then one replay over the list.  Part B groups the rows for the
// row updates at the step's end.
// Part A of `n` towers in four launches (launch_prepare_segs: the counts, the catch-up lists'
// counts and scatters; then one replay over every tower's list): the aux stream's prologue is a
// chain of small launches that the gate waits for.  ev: 2 events around the replay kernel (bench).
int towers_prepare_a(const ttamm_tower* const* T, TowerWs* const* W, int n, bool mimic, const Deferred& df,
                     hipStream_t s, void* const* ev = nullptr) {
    PrepSegs ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.target = df.step - 1;
    ps.cap = df.cap;
    ps.status = df.status;
    const CoalesceWs* wss[2] = {nullptr, nullptr};
    int64_t table_rows[2] = {0, 0};
    ReplayArgs ra = replay_header(df, df.step - 1, 0);  // stamped by the list build
    for (int k = 0; k < n; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        wss[ps.count] = &w.co;
        table_rows[ps.count] = t.id.rows;
        PrepSeg& g = ps.seg[ps.count++];
        g.idx = w.idx;
        g.n = w.R;
        g.cnt = w.co.cnt;
        g.first = w.co.first;
        if (!df.on || w.R == 0) continue;
        const ttamm_table* tabs[2];
        const int nt = dense_tables(t, mimic, tabs);
        if (nt == 0) continue;
        TTAMM_REQUIRE(w.cl.cnt != nullptr, "deferred AdamW: catch-up list workspace missing");
        g.list_cnt = w.cl.cnt;
        g.list_rows = w.cl.rows;
        g.list_lag = w.cl.lag;
        g.nlast = nt;
        for (int i = 0; i < nt; ++i) {
            g.last[i] = tabs[i]->last_step;
            ReplaySeg r = replay_seg(*tabs[i]);
            r.row_lo = 0;
            r.row_hi = w.R;
            r.list_rows = w.cl.rows;
            r.list_lag = w.cl.lag;
            r.list_cnt = w.cl.cnt;
            ra.seg[ra.count++] = r;
        }
    }
    int rc;
    if ((rc = launch_prepare_segs(ps, wss, table_rows, s))) return rc;
    return launch_replay(ra, s, ev);
}

int tower_prepare(const ttamm_tower& t, TowerWs& w, bool mimic, const Deferred& df, hipStream_t s,
                  void* const* ev = nullptr) {
    int rc;
    const ttamm_tower* T[1] = {&t};
    TowerWs* W[1] = {&w};
    if ((rc = towers_prepare_a(T, W, 1, mimic, df, s, ev))) return rc;
    return launch_coalesce_group(w.idx, w.R, t.id.rows, w.co, s);  // part B
}

// Fork / join events of the aux stream, one set per host thread, device and aux stream (reused
// across steps: a wait binds to the record that precedes it; per aux stream, so the engines of
// in-process ranks — each with its own aux stream — never wait on one another's records).
enum AuxEvent {
    EV_FORK = 0,  // main: the aux prologue may start
    EV_CURRENT,   // aux: the batch's rows are current (before the fusion)
    EV_GROUPED,   // aux: the batch's rows are grouped (before the table updates)
    EV_TO_AUX,    // main: the tables are the aux stream's (after the fusion backward; at a flush)
    EV_FROM_AUX,  // aux: its table writes are done (joined at the step's / the flush's end)
    kAuxEvents
};
// Device-scope fork / join: both streams are on this device, so an agent-scope release / acquire
// (what every kernel boundary already does) orders their memory.  The default system-scope fence
// of an event record / wait added ≈2 µs of main-stream idle at each of the step's event
// operations (an L2 writeback + invalidate per event, profiles/r06_s23_*).
constexpr unsigned kSyncEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
hipError_t create_sync_event(hipEvent_t* e) {
    const hipError_t rc = hipEventCreateWithFlags(e, kSyncEventFlags);
    if (rc != hipErrorInvalidValue) return rc;
    (void)hipGetLastError();  // a runtime without the flag: the system-scope event
    return hipEventCreateWithFlags(e, hipEventDisableTiming);
}
int aux_events(hipEvent_t ev[kAuxEvents], hipStream_t aux) {
    struct Set {
        int dev;
        hipStream_t aux;
        hipEvent_t e[kAuxEvents];
    };
    thread_local std::vector<Set> cache;
    int dev = 0;
    TTAMM_HIP(hipGetDevice(&dev));
    for (const Set& p : cache)
        if (p.dev == dev && p.aux == aux) {
            for (int i = 0; i < kAuxEvents; ++i) ev[i] = p.e[i];
            return TTAMM_OK;
        }
    Set p;
    p.dev = dev;
    p.aux = aux;
    for (int i = 0; i < kAuxEvents; ++i) TTAMM_HIP(create_sync_event(&p.e[i]));
    cache.push_back(p);
    for (int i = 0; i < kAuxEvents; ++i) ev[i] = p.e[i];
    return TTAMM_OK;
}

// A deferred dense ID table is read by the step's first gather, which must then follow the
// catch-up of its rows: nothing to run beside, the step stays on one stream.
bool overlapped(const ttamm_step_args& A, const Deferred& df) {
    return !(df.on && (A.user.id.optimizer == TTAMM_OPT_DENSE || A.item.id.optimizer == TTAMM_OPT_DENSE));
}

// Where the launches of one ABI call (train step, phase call, flush) go — the caller's stream `s`
// or the aux stream — and what orders the two.  Built once per call by stream_plan.  Invariant:
//  (a) Whatever a call enqueues on `aux` that writes state the caller may read after syncing `s`
//      (tables, moments, last_step, steps_applied, the history ring) is joined to `s` before the
//      call returns: the catch-up by EV_CURRENT, which the fusion waits for; the row updates, the
//      loss and the step-begin by EV_FROM_AUX, rows_beside_mlp's last operation.
//  (b) The rolling slice needs no join of its own: the next catch-up or flush runs on `aux` behind
//      it and supersedes it.  (`slice` implies `rows` — clipping needs dense ID tables, and deferred
//      ones leave no fork — so (a)'s join happens to cover it.)
//  (c) A flush orders `aux` behind `s` before its replay, then `s` behind `aux` — unless
//      `tables_on_aux`: the steps' writers of the tables are on `aux` already.
// The grouping (EV_GROUPED) writes workspace only; its readers on `s` wait for it (join_grouping),
// in a later phase call if need be.
struct StreamPlan {
    int rc;           // TTAMM_OK, or why the aux events could not be made
    hipStream_t s;
    hipStream_t aux;  // null: no usable aux stream, every launch goes to s
    hipEvent_t ev[kAuxEvents];
    // index prologue (gather, catch-up, grouping) on aux beside the feature MLP: see overlapped
    const bool fork;
    // bf16 towers fork after the first layer's GEMM (its one-block-per-CU tiles otherwise wait for
    // CUs behind the catch-up replay), and their ID gather stays on s
    const bool late_fork;
    // one process, deferred: the previous step's rolling slice on aux, beside the GEMMs (sharded:
    // it closes the table updates, on their stream)
    const bool slice;
    // touched-row updates on aux beside the MLP backward, joined at the call's end (one process: the
    // loss finalize and the step-begin with them; sharded: TOWERS_BWD with item rows, the other
    // phases update on s).  Not with clipping: the updates wait for the global norm.
    const bool rows;
    // one process with `rows`: every writer of the tables runs on aux (s only reads them, before
    // EV_TO_AUX), so a flush there follows them without waiting for the tail of s
    const bool tables_on_aux;
};

StreamPlan stream_plan(const ttamm_step_args& A, const Deferred& df, bool clip_on, hipStream_t s) {
    hipStream_t a = static_cast<hipStream_t>(A.aux_stream);
    hipStream_t aux = (a != nullptr && a != s) ? a : nullptr;
    const bool fork = aux != nullptr && overlapped(A, df);
    const bool rows = fork && !clip_on && (!sharded(A) || A.n_item_rows > 0);
    StreamPlan p{TTAMM_OK, s, aux, {}, fork, fork && A.user.matmul_bf16 != 0, fork && df.on && !sharded(A), rows,
                 rows && !sharded(A)};
    if (aux) p.rc = aux_events(p.ev, aux);
    return p;
}

// tower_prepare of `n` towers, then their forward.  With pl.fork the index-only prologue runs on
// the aux stream while `s` runs the feature MLP: part A (count + deferred catch-up) first, joined
// before the fusion, whose epilogue reads the mimic rows; then part B (grouping), joined by
// table_updates.
// cu_events (optional): ttamm_step_args.timing_events + 8 — [0, 1] around the user tower's
// catch-up replay, [2, 3] around the item tower's (overlapped: [0, 1] around the one replay of
// both towers' lists)
int prepare_forward(const ttamm_tower* T[2], TowerWs* W[2], int n, const ttamm_batch& bt, int D, bool mimic,
                    const Deferred& df, const StreamPlan& pl, void* const* l0_events,
                    void* const* maint_events = nullptr, void* const* cu_events = nullptr,
                    void* const* gather_events = nullptr) {
    int rc;
    const hipStream_t s = pl.s, aux = pl.aux;
    const hipEvent_t* ev = pl.ev;
    auto cu_ev = [&](int k) -> void* const* {
        return cu_events ? cu_events + (W[k]->role == ROLE_USER ? 0 : 2) : nullptr;
    };
    if (!pl.fork) {
        for (int k = 0; k < n; ++k)
            if ((rc = tower_prepare(*T[k], *W[k], mimic, df, s, cu_ev(k)))) return rc;
        return tower_forward(T, W, bt, D, mimic, s, n, l0_events, FWD_ALL);
    }
    // The MLP launches are enqueued first: the prologue is a dozen small launches whose
    // host-side enqueue would otherwise hold the GEMMs back behind the host.
    // fp32 towers: the ID-row gather also runs on the aux stream (ahead of the catch-up), beside the
    // first-layer GEMM, which reads only the feature rows; the fusion joins it with the catch-up
    const bool gather_aux = !pl.late_fork;
    if (!pl.late_fork) TTAMM_HIP(hipEventRecord(ev[EV_FORK], s));
    if ((rc = tower_forward(T, W, bt, D, mimic, s, n, l0_events, gather_aux ? FWD_FEAT : FWD_MLP,
                            pl.late_fork ? ev[EV_FORK] : nullptr)))
        return rc;
    TTAMM_HIP(hipStreamWaitEvent(aux, ev[EV_FORK], 0));
    if (gather_aux) {
        const bool timed = gather_events && gather_events[0] && gather_events[1];
        if (timed) TTAMM_HIP(hipEventRecord((hipEvent_t)gather_events[0], aux));
        if ((rc = tower_forward(T, W, bt, D, mimic, aux, n, nullptr, FWD_GATHER))) return rc;
        if (timed) TTAMM_HIP(hipEventRecord((hipEvent_t)gather_events[1], aux));
    }
    if ((rc = towers_prepare_a(T, W, n, mimic, df, aux, cu_ev(0)))) return rc;
    TTAMM_HIP(hipEventRecord(ev[EV_CURRENT], aux));
    // the fusion is enqueued before the grouping's dozen launches: enqueued after them, the host
    // still issued them when the GPU finished the MLP (~55 us idle per C2 step)
    TTAMM_HIP(hipStreamWaitEvent(s, ev[EV_CURRENT], 0));
    if ((rc = tower_forward(T, W, bt, D, mimic, s, n, l0_events, FWD_FUSION))) return rc;
    for (int k = 0; k < n; ++k)  // part B
        if ((rc = launch_coalesce_group(W[k]->idx, W[k]->R, T[k]->id.rows, W[k]->co, aux))) return rc;
    TTAMM_HIP(hipEventRecord(ev[EV_GROUPED], aux));
    if (pl.slice) {
        // The previous step's slice (target step - 1), behind this step's catch-up on the aux
        // stream, overlapping the main stream's GEMMs instead of closing the step.  The rows this
        // batch touches are current to step - 1 after the catch-up, so the slice skips them and
        // never races the row updates; its stamp is an atomicMax (a row update may have moved a
        // row to `step` meanwhile).  The next step's catch-up and the flush run on the aux stream
        // too, after it, and supersede it (StreamPlan (b)).
        if ((rc = replay_slice(T, n, mimic, df, df.step - 1, 2, maint_events, aux))) return rc;
    }
    return TTAMM_OK;
}

// the row updates on `s` need the grouping (prepare part B), which a fork left on the aux stream
int join_grouping(const StreamPlan& pl) {
    if (pl.fork) TTAMM_HIP(hipStreamWaitEvent(pl.s, pl.ev[EV_GROUPED], 0));
    return TTAMM_OK;
}

RowUpdateArgs row_update_args(const ttamm_tower& t, TowerWs& w, int D, bool mimic, const SparseConsts& sp,
                              const AdamConsts& ad, const Deferred& df, const float* grad_scale) {
    RowUpdateArgs ru;
    std::memset(&ru, 0, sizeof(ru));
    ru.n = w.R;
    ru.dim = t.id.dim;  // == D unless concat fusion has another output_dim (tower_optimizer_rows)
    ru.n_unique = w.co.n_unique;
    ru.seg_start = w.co.seg_start;
    ru.keys = w.co.keys_out;
    ru.rows = w.co.vals_out;
    ru.seglong = w.co.seglong;
    if (uses_ef(t)) {
        ru.dE = w.dEF;
        ru.ld_dE = efw(t);
    } else {
        ru.dE = w.dT;
        ru.ld_dE = w.dT_ld;
    }
    ru.id = t.id;
    if (mimic) {
        ru.mimic = t.mimic;
        ru.dA_lo = w.dA;
        ru.dA_hi = w.dT;
        ru.ld_dA = w.dA_ld;
        ru.split_row = w.dA_split;
        ru.xu = w.xu;
    }
    ru.side_id = w.side_id;
    ru.side_mimic = w.side_mimic;
    ru.piece_e = w.piece_e;
    ru.piece_a = w.piece_a;
    ru.sp = sp;
    ru.ad = ad;
    ru.dense_step = df.step;
    ru.status = df.status;
    ru.grad_scale = grad_scale;
    return ru;
}
int tower_optimizer_rows(const ttamm_tower& t, TowerWs& w, int D, bool mimic, const SparseConsts& sp,
                         const AdamConsts& ad, const Deferred& df, hipStream_t s, const float* grad_scale) {
    const RowUpdateArgs ru = row_update_args(t, w, D, mimic, sp, ad, df, grad_scale);
    if (!mimic || t.id.dim == D) return launch_row_update(ru, s);
    // concat with output_dim != embedding_dim: the ID rows and the (output-wide) mimic rows differ
    // in width, so the two tables are updated by two passes over the same row grouping
    RowUpdateArgs a = ru, b = ru;
    std::memset(&a.mimic, 0, sizeof(a.mimic));
    a.piece_a = a.side_mimic = nullptr;
    std::memset(&b.id, 0, sizeof(b.id));
    b.dE = nullptr;
    b.piece_e = b.side_id = nullptr;
    b.dim = D;
    int rc;
    if ((rc = launch_row_update(a, s))) return rc;
    return launch_row_update(b, s);
}
void add_seg(SweepArgs& sw, const ttamm_table& tb) {
    sw.seg[sw.count].p = tb.weight;
    sw.seg[sw.count].m = tb.exp_avg;
    sw.seg[sw.count].v = tb.exp_avg_sq;
    sw.seg[sw.count].n = tb.rows * tb.dim;
    sw.count++;
}

// What bind_rows derives from the arguments of one ABI call, for run_single and run_phases.
struct Step {
    const ttamm_step_args& A;
    StepWs ws;
    int D = 0;
    bool mimic = false;
    int64_t B = 0, Bg = 0;  // this call's batch, the global batch
    int N = 0;
    int64_t num_items = 0;
    int64_t* neg = nullptr;  // where the sampler writes the negatives
    const ttamm_tower* T[2] = {};
    TowerWs* W[2] = {};  // {&ws.user, &ws.item}
    AdamConsts ad{};
    SparseConsts sp{};
    Deferred df;
    explicit Step(const ttamm_step_args& a) : A(a) {}
};

// Touched-row updates of the tables of `n` towers, then the AdamW(g=0) step of the rows the
// batch did not touch: eagerly, one sweep over the dense-group tables and a scatter of the
// staged touched rows; deferred, the replay of this step's 1/slices of the rows to `step`.
// on_aux: on the aux stream, behind the grouping there (rows_beside_mlp); else on pl.s.
int table_updates(const Step& c, const ttamm_tower* T[2], TowerWs* W[2], int n, const StreamPlan& pl, bool on_aux,
                  void* const events[2], const float* grad_scale = nullptr) {
    const int D = c.D;
    const bool mimic = c.mimic;
    const AdamConsts& ad = c.ad;
    const Deferred& df = c.df;
    const hipStream_t s = on_aux ? pl.aux : pl.s;
    int rc;
    if (!on_aux && (rc = join_grouping(pl))) return rc;
    for (int k = 0; k < n; ++k)
        if ((rc = tower_optimizer_rows(*T[k], *W[k], D, mimic, c.sp, ad, df, s, grad_scale))) return rc;
    if (df.on) {
        if (pl.slice) return TTAMM_OK;  // replayed on the aux stream (prepare_forward)
        return replay_slice(T, n, mimic, df, df.step, 1, events, s);
    }
    SweepArgs sw;
    std::memset(&sw, 0, sizeof(sw));
    sw.ad = ad;
    sw.status = df.status;
    if (mimic)
        for (int k = 0; k < n; ++k) add_seg(sw, T[k]->mimic);
    for (int k = 0; k < n; ++k)
        if (T[k]->id.optimizer == TTAMM_OPT_DENSE) add_seg(sw, T[k]->id);
    // SGD without momentum or weight decay leaves g = 0 rows where they are: no sweep
    const bool sweep = !(ad.sgd && ad.sgd_mom == 0.f && ad.wd == 0.f);
    if (events && events[0]) TTAMM_HIP(hipEventRecord((hipEvent_t)events[0], s));
    if (sweep && (rc = launch_dense_sweep(sw, s))) return rc;
    if (events && events[1]) TTAMM_HIP(hipEventRecord((hipEvent_t)events[1], s));
    for (int k = 0; k < n; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (mimic)
            if ((rc = launch_side_scatter(w.co.n_unique, w.co.keys_out, w.co.seg_start, w.side_mimic, w.R, D, t.mimic,
                                          df.status, s)))
                return rc;
        if (t.id.optimizer == TTAMM_OPT_DENSE)
            if ((rc = launch_side_scatter(w.co.n_unique, w.co.keys_out, w.co.seg_start, w.side_id, w.R, t.id.dim, t.id,
                                          df.status, s)))
                return rc;
    }
    return TTAMM_OK;
}

DenseAdamArgs dense_args(const ttamm_tower* T[2], TowerWs* W[2], const AdamConsts& ad, const uint32_t* status,
                         const float* grad_scale) {
    DenseAdamArgs da;
    std::memset(&da, 0, sizeof(da));
    da.ad = ad;
    da.status = status;
    da.grad_scale = grad_scale;
    auto add_dense = [&](float* p, float* m, float* v, const float* g, int64_t n) {
        da.t[da.count++] = DenseTensor{p, m, v, g, n};
    };
    for (int k = 0; k < 2; ++k) {
        const ttamm_tower& t = *T[k];
        TowerWs& w = *W[k];
        if (t.fusion == TTAMM_FUSION_IDENTITY) continue;
        for (int l = 0; l < t.n_linear; ++l) {
            const ttamm_linear& L = t.linear[l];
            add_dense(L.weight, L.weight_exp_avg, L.weight_exp_avg_sq, w.gw[l], (int64_t)L.out_features * L.in_features);
            add_dense(L.bias, L.bias_exp_avg, L.bias_exp_avg_sq, w.gb[l], L.out_features);
        }
        {
            for (int q = 0; q < fusion_linears(t); ++q) {
                const ttamm_linear& L = t.gate[q];
                add_dense(L.weight, L.weight_exp_avg, L.weight_exp_avg_sq, w.ggw[q],
                          (int64_t)L.out_features * L.in_features);
                add_dense(L.bias, L.bias_exp_avg, L.bias_exp_avg_sq, w.ggb[q], L.out_features);
            }
        }
    }
    return da;
}
int dense_update(const ttamm_tower* T[2], TowerWs* W[2], const AdamConsts& ad, const uint32_t* status, hipStream_t s,
                 const float* grad_scale = nullptr) {
    return launch_dense_adam(dense_args(T, W, ad, status, grad_scale), s);
}

// the tables' row partials of the squared gradient norm into ws.clip_partials[1, *off)
int clip_table_partials(Step& c, const StreamPlan& pl, int* off_out) {
    StepWs& ws = c.ws;
    int rc;
    if ((rc = join_grouping(pl))) return rc;  // the row grouping
    int off = 1;
    for (int k = 0; k < 2; ++k) {
        if (c.W[k]->R <= 0) continue;
        const RowUpdateArgs ru = row_update_args(*c.T[k], *c.W[k], c.D, c.mimic, c.sp, c.ad, c.df, nullptr);
        if ((rc = launch_rows_sumsq(ru, ws.clip_partials + off, pl.s))) return rc;
        off += rows_sumsq_blocks(c.W[k]->R, c.T[k]->id.dim);
    }
    TTAMM_REQUIRE(off <= ws.clip_parts, "clip: partials overflow");
    *off_out = off;
    return TTAMM_OK;
}

// clip_grad_norm_(model.parameters(), max_norm) (training.py:824-825): the global gradient norm
// over both towers' table rows and dense tensors -> ws.clip_coef, read by the optimizer kernels
int clip_coefficient(Step& c, const StreamPlan& pl) {
    StepWs& ws = c.ws;
    int rc;
    int off;
    if ((rc = clip_table_partials(c, pl, &off))) return rc;
    if ((rc = launch_dense_sumsq(dense_args(c.T, c.W, c.ad, c.A.status, nullptr), ws.clip_partials + off, pl.s)))
        return rc;
    off += kDenseSumsqBlocks;
    TTAMM_REQUIRE(off <= ws.clip_parts, "clip: partials overflow");
    return launch_clip_coef(ws.clip_partials + 1, off - 1, (float)c.A.hp.grad_clip_norm, ws.clip_coef, pl.s);
}

// sharded clipping, TOWERS_BWD: this rank's share of the squared gradient norm over the table
// rows it owns (its users', its items' — every requester's contributions to a row summed first),
// into *A.table_sumsq for the caller's all-reduce
int clip_table_share(Step& c, const StreamPlan& pl) {
    int rc;
    int off;
    if ((rc = clip_table_partials(c, pl, &off))) return rc;
    return launch_sum_partials(c.ws.clip_partials + 1, off - 1, c.A.table_sumsq, pl.s);
}

// sharded clipping, TABLES: clip_grad_norm_'s coefficient from the all-reduced table share and the
// (all-reduced) replicated-weight gradients
int clip_coefficient_sharded(Step& c, hipStream_t s) {
    StepWs& ws = c.ws;
    int rc;
    TTAMM_HIP(hipMemcpyAsync(ws.clip_partials, c.A.table_sumsq, sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = launch_dense_sumsq(dense_args(c.T, c.W, c.ad, c.A.status, nullptr), ws.clip_partials + 1, s))) return rc;
    return launch_clip_coef(ws.clip_partials, 1 + kDenseSumsqBlocks, (float)c.A.hp.grad_clip_norm, ws.clip_coef, s);
}

// Deferred mode is all-or-nothing over the dense-group tables of both towers.
int deferred_of(const ttamm_step_args& A, Deferred& df) {
    const bool mimic = A.mimic_enabled != 0;
    int with = 0, total = 0;
    for (const ttamm_tower* t : {&A.user, &A.item}) {
        const ttamm_table* tabs[2];
        const int n = dense_tables(*t, mimic, tabs);
        for (int i = 0; i < n; ++i) {
            ++total;
            with += tabs[i]->last_step != nullptr ? 1 : 0;
        }
    }
    if (with == 0) return TTAMM_OK;
    TTAMM_REQUIRE(with == total, "deferred AdamW: every dense-group table needs last_step");
    TTAMM_REQUIRE(A.adam_history != nullptr && A.replay_slices >= 1 && A.history_capacity > A.replay_slices &&
                      A.history_capacity <= kMaxAdamHistory,
                  "deferred AdamW: needs adam_history and replay_slices < history_capacity <= 512");
    TTAMM_REQUIRE(A.hp.dense_step < (double)INT32_MAX, "deferred AdamW: step count out of range");
    df.on = true;
    df.hist = static_cast<AdamConsts*>(A.adam_history);
    df.cap = A.history_capacity;
    df.slices = A.replay_slices;
    df.step = (int32_t)A.hp.dense_step;
    df.decoupled = A.hp.decoupled_weight_decay ? 1 : 0;
    df.fast = A.table_g0_math == TTAMM_G0_FAST ? 1 : 0;
    df.sgd = A.hp.dense_optimizer == TTAMM_DENSE_SGD ? 1 : 0;
    return TTAMM_OK;
}

// the category-alignment rows of this step: one process, the item tower's augmented rows
// [positives; negatives]; sharded requester, its requests' (t | a) exchange rows and global ids
CalArgs& bind_cal(Step& st) {
    const ttamm_step_args& A = st.A;
    const TowerWs& I = st.ws.item;
    const int64_t B = st.B;
    const int D = st.D;
    const bool mimic = st.mimic;
    CalArgs& c = st.ws.cal;
    c.xa_rows = INT64_MAX;
    if (sharded(A)) {
        c.x = A.item_fwd_in;
        c.xa = mimic ? A.item_fwd_in + D : nullptr;
        c.ld_x = 2 * D;
        c.slot = A.item_slot;
        if (compact_exchange(A)) {  // units of D floats; a negative's row is t + a already
            c.ld_x = D;
            c.slot = A.item_slot;  // units (ttamm_route_rows with counts_ld >= 3)
            c.xa_rows = B;
        }
        c.idx = A.b.pos_items;
        c.idx1 = A.b.neg_items;
        c.split = B;
        c.idx_rows = A.num_items_global > 0 ? A.num_items_global : A.item.id.rows;
    } else {
        c.x = I.aug;
        c.ld_x = D;
        c.idx = I.idx;
        c.idx_rows = A.item.id.rows;
    }
    c.categories = A.item_categories;
    c.num_categories = A.num_categories;
    c.major = A.major_category;
    c.lambda = (float)A.hp.lambda_category_alignment;
    return c;
}

// ... and where their gradient goes: one process, the item tower's dT / dA; sharded requester, the
// (dT | dA) rows it ships back
CalArgs& bind_cal_grads(Step& st) {
    const ttamm_step_args& A = st.A;
    const int D = st.D;
    CalArgs& c = bind_cal(st);
    if (sharded(A)) {
        c.dT = A.item_bwd_out;
        c.dA = st.mimic ? A.item_bwd_out + D : nullptr;
        c.ld_d = 2 * D;
        c.dA_rows = c.R;  // every request ships its own dA
        if (compact_exchange(A)) {  // only the positives ship a dA
            c.ld_d = D;
            c.dA_rows = st.B;
        }
    } else {
        c.dT = st.ws.item.dT_own;
        c.dA = st.mimic ? st.ws.item.dA_own : nullptr;
        c.ld_d = D;
        c.dA_rows = st.B;
    }
    return c;
}

// in-batch negatives: the positives every user is scored against; the BCE terms of the step
int64_t inbatch_cols(const Step& st) { return st.ws.ib_on ? (sharded(st.A) ? st.Bg : st.B) : 0; }
// (softmax: the mean is over the B rows' terms)
int64_t bce_count(const Step& st) {
    return st.ws.ib_softmax ? st.B : st.Bg * ((st.ws.ib_on ? inbatch_cols(st) : 1) + st.N);
}

// S = U P^T, its BCE, dU and dP: one process against the batch's own positives, sharded against
// every rank's (inbatch_items)
InBatchArgs& bind_inbatch(Step& st) {
    const ttamm_step_args& A = st.A;
    const bool shard = sharded(A);
    const int D = st.D;
    InBatchArgs& a = st.ws.ib;
    const float* P = shard ? A.inbatch_items : st.ws.item.aug;  // one process: rows [0, B), the positives
    static_cast<InBatchProblem&>(a) = {st.ws.user.aug, D, st.B, P, D, inbatch_cols(st), D, shard ? A.row_base : 0};
    a.inv_T = 1.0f / (float)bce_count(st);
    a.dU = st.ws.ib_du;
    a.ld_du = D;
    a.dP = shard ? A.inbatch_dp_all : st.ws.ib_dp;
    a.ld_dp = D;
    return a;
}
int run_inbatch(Step& st, hipStream_t s) {
    int rc;
    void* const* ev = st.A.timing_events + 4;
    if (ev[0] && ev[1]) TTAMM_HIP(hipEventRecord((hipEvent_t)ev[0], s));
    InBatchArgs& a = bind_inbatch(st);
    if (st.ws.ib_softmax) {  // the LSE pass (the rows' normalisers, the loss partials), then the softmax gradient kernel
        InBatchLossArgs& l = st.ws.ib_lse;
        static_cast<InBatchProblem&>(l) = a;
        if ((rc = launch_inbatch_softmax(a, l, st.A.in_batch_inv_temperature, s))) return rc;
    } else if ((rc = launch_inbatch(a, s))) {
        return rc;
    }
    if (ev[0] && ev[1]) TTAMM_HIP(hipEventRecord((hipEvent_t)ev[1], s));
    return TTAMM_OK;
}

// scores, BCE and mimic MSE with their gradient seeds: one process on the item tower's rows,
// sharded requester on the exchange rows it received / ships back
ScoreArgs bind_score(Step& st) {
    const ttamm_step_args& A = st.A;
    const TowerWs &U = st.ws.user, &I = st.ws.item;
    const int D = st.D;
    const bool mimic = st.mimic;
    ScoreArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.B = st.B;
    sa.Bg = st.Bg;
    sa.N = st.N;
    sa.D = D;
    sa.user_aug = U.aug;
    sa.t_user = U.t;
    sa.a_user = U.a;
    sa.lambda_u = (float)A.hp.lambda_mimic_user;
    sa.lambda_i = (float)A.hp.lambda_mimic_item;
    sa.mimic = mimic ? 1 : 0;
    sa.dT_user = U.dT_own;
    sa.dA_user = U.dA_own;
    if (sharded(A)) {
        sa.item_aug = nullptr;
        sa.t_item = A.item_fwd_in;
        sa.a_item = mimic ? A.item_fwd_in + D : nullptr;
        sa.ld_item = 2 * D;
        sa.dT_item = A.item_bwd_out;
        sa.dA_item = mimic ? A.item_bwd_out + D : nullptr;
        sa.dA_all = 1;
        sa.ld_dti = 2 * D;
        sa.item_slot = A.item_slot;
        if (compact_exchange(A)) {  // D-float units; negatives: t + a in, dT out (their dA is dT)
            sa.ld_item = sa.ld_dti = D;
            sa.dA_all = 0;
            sa.neg_aug = 1;
        }
    } else {
        sa.item_aug = I.aug;
        sa.t_item = I.t;
        sa.a_item = I.a;
        sa.ld_item = D;
        sa.dT_item = I.dT_own;
        sa.dA_item = I.dA_own;
        sa.ld_dti = D;
    }
    sa.partials = st.ws.partials;
    sa.blocks = st.ws.score_blocks;
    sa.inv_numel = 1.0f / (float)bce_count(st);
    if (st.ws.ib_on) {
        sa.ib_du = st.ws.ib_du;
        sa.ib_dp = sharded(A) ? A.inbatch_dp : st.ws.ib_dp;
        sa.ib_ld = D;
    }
    return sa;
}

int loss_finalize(const Step& st, hipStream_t s) {
    const ttamm_step_args& A = st.A;
    const StepWs& ws = st.ws;
    if (!A.loss_out) return TTAMM_OK;
    // softmax: the LSE pass's block partials (the scorer adds no retrieval term with N = 0)
    const float* ib_part = ws.ib_softmax ? ws.ib_lse.loss_part : ws.ib_on ? ws.ib.loss_part : nullptr;
    const int ib_parts = ws.ib_softmax ? inbatch_lse_parts(st.B) : ws.ib_on ? ws.ib_parts : 0;
    return launch_loss_finalize(ws.partials, ws.score_blocks, ib_part, ib_parts, bce_count(st), st.B, st.Bg, st.D,
                                (float)A.hp.lambda_mimic_user, (float)A.hp.lambda_mimic_item, st.mimic ? 1 : 0,
                                ws.cal_on && A.row_base == 0 ? ws.cal.out : nullptr,
                                (float)A.hp.lambda_category_alignment, A.loss_out, A.loss_accum, A.status, s);
}

int validate_step(const ttamm_step_args& A) {
    const int D = out_dim(A.user);
    int rc;
    TTAMM_REQUIRE(A.table_g0_math == TTAMM_G0_EXACT || A.table_g0_math == TTAMM_G0_FAST,
                  "table_g0_math must be TTAMM_G0_EXACT or TTAMM_G0_FAST");
    if ((rc = validate_pair(A, true))) return rc;
    if (A.hp.grad_clip_norm > 0.0 && A.mimic_enabled)
        TTAMM_REQUIRE(A.user.id.dim == D && A.item.id.dim == D,
                      "gradient clipping with a concat output_dim other than the embedding dim is not supported");
    TTAMM_REQUIRE(A.b.batch > 0, "empty batch");
    if (cal_enabled(A)) {
        TTAMM_REQUIRE(!sharded(A) || (A.cal_stats && A.cal_scatter),
                      "the row-sharded category-alignment loss needs cal_stats and cal_scatter");
        TTAMM_REQUIRE(!sharded(A) || !(A.phase & (TTAMM_PHASE_CAL_STATS | TTAMM_PHASE_CAL_SCATTER |
                                                  TTAMM_PHASE_SCORE | TTAMM_PHASE_USER)) ||
                          (A.item_fwd_in && (A.b.num_neg == 0 || A.b.neg_items)),
                      "the row-sharded category-alignment loss needs item_fwd_in and b.neg_items");
        TTAMM_REQUIRE(A.num_categories > 0 && A.num_categories <= 65535,
                      "category alignment: num_categories must be in [1, 65535]");
        TTAMM_REQUIRE(A.major_category >= 0 && A.major_category < A.num_categories,
                      "category alignment: major_category out of range");
        TTAMM_REQUIRE(D <= 256, "category alignment: embedding dim must be <= 256");
    }
    TTAMM_REQUIRE(A.in_batch_loss == TTAMM_INBATCH_BCE || A.in_batch_loss == TTAMM_INBATCH_SOFTMAX,
                  "in_batch_loss must be 0 (the BCE mean) or 1 (the softmax cross-entropy)");
    if (A.in_batch_loss != TTAMM_INBATCH_BCE) {
        TTAMM_REQUIRE(!sharded(A),
                      "in_batch_loss: the softmax objective needs phase == 0, the whole step in one call (it is not "
                      "built for the row-sharded step)");
        TTAMM_REQUIRE(A.in_batch != 0, "in_batch_loss: the softmax objective needs in_batch");
        TTAMM_REQUIRE(A.b.num_neg == 0,
                      "in_batch_loss: the softmax objective needs b.num_neg == 0 (sampled negatives do not join the "
                      "denominator)");
        if ((rc = inbatch_softmax_check(A.in_batch_inv_temperature))) return rc;
    }
    if (A.in_batch) {
        TTAMM_REQUIRE(A.b.num_neg >= 0, "num_negatives must be >= 0 with in-batch negatives");
        TTAMM_REQUIRE(D % 4 == 0 && D <= 128, "in-batch negatives: embedding dim must be <= 128");
    } else {
        TTAMM_REQUIRE(A.b.num_neg > 0, "num_negatives must be greater than zero.");
    }
    const int64_t num_items = A.num_items_global > 0 ? A.num_items_global : A.item.id.rows;
    TTAMM_REQUIRE(num_items > 1, "num_items must be greater than one.");
    if ((rc = validate_mimic_pair(A))) return rc;
    TTAMM_REQUIRE(A.hp.dense_step >= 1 && A.hp.sparse_step >= 1, "optimizer step counts must be >= 1");
    TTAMM_REQUIRE(A.hp.dense_optimizer == TTAMM_DENSE_ADAM || A.hp.dense_optimizer == TTAMM_DENSE_SGD,
                  "hp.dense_optimizer must be TTAMM_DENSE_ADAM or TTAMM_DENSE_SGD");
    for (const ttamm_tower* t : {&A.user, &A.item})
        if (t->id.max_norm > 0.0) {
            TTAMM_REQUIRE(t->id.optimizer == TTAMM_OPT_DENSE, "max_norm is not supported when using sparse embeddings.");
        }
    if (A.hp.grad_clip_norm > 0.0) {
        TTAMM_REQUIRE(!sharded(A) || !(A.phase & (TTAMM_PHASE_USER | TTAMM_PHASE_ITEM_BWD)),
                      "gradient clipping in the row-sharded step needs the grouped schedule (SCORE / TOWERS_BWD)");
        TTAMM_REQUIRE(!sharded(A) || A.table_sumsq != nullptr, "sharded gradient clipping needs table_sumsq");
        TTAMM_REQUIRE(A.user.id.optimizer == TTAMM_OPT_DENSE && A.item.id.optimizer == TTAMM_OPT_DENSE,
                      "gradient clipping needs dense ID tables (clip_grad_norm_ cannot take the sparse gradients "
                      "of sparse ID tables)");
    }
    TTAMM_REQUIRE(A.row_base >= 0 && (A.global_batch == 0 || A.global_batch >= A.row_base + A.b.batch),
                  "row_base / global_batch out of range");
    if (!sharded(A)) return TTAMM_OK;
    const int ph = A.phase;
    TTAMM_REQUIRE((ph & ~8191) == 0, "unknown phase bits");
    TTAMM_REQUIRE(!((ph & TTAMM_PHASE_USER) && (ph & (TTAMM_PHASE_SCORE | TTAMM_PHASE_TOWERS_BWD))),
                  "USER and SCORE / TOWERS_BWD are alternatives");
    TTAMM_REQUIRE(A.in_batch || (ph & (TTAMM_PHASE_INBATCH_SRC | TTAMM_PHASE_INBATCH)) == 0,
                  "INBATCH phases need in_batch");
    TTAMM_REQUIRE(A.item_rows_capacity >= 0 && A.n_item_rows >= 0 && A.n_item_rows <= A.item_rows_capacity,
                  "n_item_rows exceeds item_rows_capacity");
    if (ph & TTAMM_PHASE_SAMPLE)
        TTAMM_REQUIRE(!A.b.sample_negatives || A.b.neg_items, "sharded SAMPLE phase needs b.neg_items for the exchange");
    if (A.exchange_counts) {
        TTAMM_REQUIRE(A.mimic_enabled && A.item.fusion == TTAMM_FUSION_GATED,
                      "compact exchange rows (exchange_counts) need mimic on and a gated item tower");
        TTAMM_REQUIRE(A.exchange_world >= 1 && A.exchange_world <= 1024 && A.exchange_counts_ld >= 3,
                      "exchange_counts needs exchange_world in [1, 1024] and exchange_counts_ld >= 3");
        TTAMM_REQUIRE(A.item_slot, "compact exchange rows need item_slot (the requests' units)");
    }
    if ((ph & (TTAMM_PHASE_ITEM_FWD | TTAMM_PHASE_ITEM_BWD)) && A.n_item_rows > 0)
        TTAMM_REQUIRE(A.item_rows && A.item_row_keys, "item_rows / item_row_keys missing");
    if (ph & TTAMM_PHASE_ITEM_FWD) TTAMM_REQUIRE(A.item_fwd_out || A.n_item_rows == 0, "item_fwd_out missing");
    if (ph & (TTAMM_PHASE_USER | TTAMM_PHASE_SCORE))
        TTAMM_REQUIRE(A.item_fwd_in && A.item_bwd_out, "item_fwd_in / item_bwd_out missing");
    if (ph & (TTAMM_PHASE_ITEM_BWD | TTAMM_PHASE_TOWERS_BWD))
        TTAMM_REQUIRE(A.item_bwd_in || A.n_item_rows == 0, "item_bwd_in missing");
    if (ph & (TTAMM_PHASE_USER | TTAMM_PHASE_SCORE | TTAMM_PHASE_ITEM_BWD | TTAMM_PHASE_TOWERS_BWD |
              TTAMM_PHASE_DENSE))
        TTAMM_REQUIRE(A.dense_grads != nullptr, "dense_grads missing");
    return TTAMM_OK;
}

// The shared preamble of a step call: validate, lay out the workspace, bind the towers' rows to
// it (sharded: the item tower's to the caller's exchange buffers), form the optimizers' constants.
int bind_rows(Step& c) {
    const ttamm_step_args& A = c.A;
    int rc;
    if ((rc = validate_step(A))) return rc;
    const int D = c.D = out_dim(A.user);
    const bool mimic = c.mimic = A.mimic_enabled != 0;
    const bool shard = sharded(A);

    Arena ar{static_cast<char*>(A.workspace), A.workspace_bytes, 0, false};
    plan(ar, A, c.ws);
    TTAMM_REQUIRE(ar.ok(), "workspace too small for this step");

    const int64_t B = c.B = A.b.batch;
    const int N = c.N = A.b.num_neg;
    const int64_t Bg = c.Bg = global_batch(A);
    c.num_items = A.num_items_global > 0 ? A.num_items_global : A.item.id.rows;
    TowerWs& U = c.ws.user;
    TowerWs& I = c.ws.item;
    U.idx = U.fidx = U.idx_own;  // staged copy of A.b.users
    U.key_split = B;
    U.key_base0 = A.row_base;
    if (shard) {
        I.R = A.n_item_rows;
        I.idx = I.fidx = I.idx_own;  // staged copy of A.item_rows
        I.row_key = c.ws.keys_own;  // staged copy of A.item_row_keys (ITEM_FWD)
        I.t = A.item_fwd_out;
        I.a = mimic && A.item_fwd_out ? A.item_fwd_out + D : nullptr;
        I.t_ld = 2 * D;
        I.aug = nullptr;
        I.dT = A.item_bwd_in;
        I.dT_ld = 2 * D;
        I.dA = A.item_bwd_in ? A.item_bwd_in + D : nullptr;
        I.dA_ld = 2 * D;
        I.dA_split = I.R;  // every row's mimic gradient is shipped in (dT | dA)
        if (compact_exchange(A)) {  // D-float units: (t | a) of a positive, t + a of a negative
            I.t_ld = I.dT_ld = I.dA_ld = D;
            I.xu = c.ws.own_units;
        }
        I.renorm_key_split = Bg;  // request keys: positives [0, Bg), negatives from Bg on
        c.neg = A.b.neg_items;
    } else {
        I.idx = I.fidx = I.idx_own;
        // item row r < B is interaction r's positive, else negative slot r - B
        I.key_split = B;
        I.key_base0 = A.row_base;
        I.key_base1 = Bg + A.row_base * N;
        c.neg = I.idx_own + B;
        I.renorm_split = B;
    }
    // max_norm claim tags: unique per lookup (users; positives, then negatives)
    U.renorm_tag = I.renorm_tag = (int32_t)(2 * (A.hp.dense_step % (1 << 29)) + 1);
    c.T[0] = &A.user, c.T[1] = &A.item;
    c.W[0] = &U, c.W[1] = &I;
    const ttamm_hparams& hp = A.hp;
    c.ad = hp.dense_optimizer == TTAMM_DENSE_SGD
               ? make_sgd_consts(hp.lr, hp.weight_decay, hp.momentum, hp.dampening, hp.nesterov, hp.sgd_first_step)
               : make_adam_consts(hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.decoupled_weight_decay,
                                  hp.dense_step);
    c.ad.fast_g0 = A.table_g0_math == TTAMM_G0_FAST ? 1 : 0;
    c.sp = make_sparse_consts(hp.sparse_lr, hp.sparse_beta1, hp.sparse_beta2, hp.sparse_eps, hp.sparse_step);
    if ((rc = deferred_of(A, c.df))) return rc;
    c.df.status = A.status;
    return TTAMM_OK;
}

// Indices and negatives: range-checked copies of the batch's ids (nn.Embedding raises IndexError,
// encoders.py:222-223: an out-of-range id sets TTAMM_STATUS_INDEX_OUT_OF_RANGE, is replaced by
// row 0 so no kernel reads outside a table, and the step writes nothing), the sampler and —
// begin_here — the step's count + AdamW constants (unless a status error stops it), in one launch.
// !begin_here: the caller runs launch_step_begin on the aux stream instead.
int step_prologue(Step& c, bool begin_here, hipStream_t s) {
    const ttamm_step_args& A = c.A;
    const bool shard = sharded(A);
    const int64_t B = c.B;
    const int N = c.N;
    StageArgs st;
    std::memset(&st, 0, sizeof(st));
    st.status = A.status;
    st.seg[st.count++] = StageSeg{A.b.users, c.ws.user.idx_own, B, A.user.id.rows};
    if (!shard) {
        st.seg[st.count++] = StageSeg{A.b.pos_items, c.ws.item.idx_own, B, A.item.id.rows};
        if (!A.b.sample_negatives && N > 0) {
            TTAMM_REQUIRE(A.b.neg_items != nullptr, "negatives must be given when sample_negatives == 0");
            st.seg[st.count++] = StageSeg{A.b.neg_items, c.neg, B * N, A.item.id.rows};
        }
    } else {  // requester: global item ids, checked only (the owners stage their local rows)
        st.seg[st.count++] = StageSeg{A.b.pos_items, nullptr, B, c.num_items};
        if (!A.b.sample_negatives && A.b.neg_items && N > 0)
            st.seg[st.count++] = StageSeg{A.b.neg_items, nullptr, B * N, c.num_items};
    }
    TTAMM_REQUIRE(A.status != nullptr, "the training step needs a status word");
    TTAMM_REQUIRE(!(A.b.sample_negatives && N > 0) || c.num_items > 1, "num_items must be greater than one.");
    PrologueArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    if (A.b.sample_negatives && N > 0) {
        // one process: into the item tower's rows and (when given) the caller's buffer
        pa.users = A.b.users;
        pa.user_rows = A.user.id.rows;
        pa.batch = B;
        pa.num_neg = N;
        pa.num_items = (uint64_t)c.num_items;
        pa.pos_offsets = A.b.pos_offsets;
        pa.pos_values = A.b.pos_values;
        pa.k0 = (uint32_t)A.b.seed;
        pa.k1 = (uint32_t)(A.b.seed >> 32);
        pa.counter = A.b.counter;
        pa.slot_base = A.row_base * N;
        pa.out = c.neg;
        pa.out2 = (!shard && A.b.neg_items != c.neg) ? A.b.neg_items : nullptr;
    }
    pa.cap = c.df.on ? c.df.cap : 2;
    pa.step = c.df.step;
    pa.c = c.ad;
    if (begin_here) {
        pa.done = c.ws.prologue_done;
        pa.applied = A.steps_applied;
        pa.hist = c.df.on ? c.df.hist : nullptr;
    }
    return launch_step_prologue(st, pa, s);
}

// The backward of both towers with the touched-row updates on the aux stream (pl.rows): once the
// fusion backward has formed the ID and mimic rows' gradients, the row updates run there beside
// the MLP's dgrad chain and weight gradients (memory-bound row traffic under MFMA-bound GEMMs).
// The grouping precedes them on that stream already.  The last operation joins the aux stream, so
// what follows the call on `s` — the next step's ID-row gather, the caller's all-reduce — sees the
// updated rows (StreamPlan (a)).  single: the one-process step, whose loss reduction (nothing in
// the backward reads it) goes ahead of the row updates and whose dense update closes the step;
// sharded, the DENSE phase follows the caller's all-reduce.
int rows_beside_mlp(Step& c, const StreamPlan& pl, bool single) {
    const ttamm_step_args& A = c.A;
    int rc;
    if ((rc = tower_backward(c.T, c.W, c.D, pl.s, 2, nullptr, BWD_GATE))) return rc;
    TTAMM_HIP(hipEventRecord(pl.ev[EV_TO_AUX], pl.s));
    TTAMM_HIP(hipStreamWaitEvent(pl.aux, pl.ev[EV_TO_AUX], 0));
    if (single && (rc = loss_finalize(c, pl.aux))) return rc;
    if ((rc = table_updates(c, c.T, c.W, 2, pl, true, A.timing_events))) return rc;
    TTAMM_HIP(hipEventRecord(pl.ev[EV_FROM_AUX], pl.aux));
    // single: the dense AdamW update rides in the weight gradients' slab reduce (WgradTail), the
    // same operations per element as dense_update after the plain reduce
    const DenseTail dense{c.ad, A.status};
    if ((rc = tower_backward(c.T, c.W, c.D, pl.s, 2, A.timing_events + 6, BWD_MLP, single ? &dense : nullptr))) return rc;
    TTAMM_HIP(hipStreamWaitEvent(pl.s, pl.ev[EV_FROM_AUX], 0));
    return TTAMM_OK;
}

// ---- the one-process step, in launch order ------------------------------------------------------
int run_single(Step& c, const StreamPlan& pl) {
    const ttamm_step_args& A = c.A;
    const Deferred& df = c.df;
    StepWs& ws = c.ws;
    const hipStream_t s = pl.s;
    int rc;
    // pl.rows: the step's count and AdamW constants are published by step_begin_kernel on the aux
    // stream (below) instead of by the prologue's last block, whose completion counter (a release
    // fence and an atomic per block) sat on the main stream's path to the first GEMM.  Nothing in
    // this step reads this step's history entry (the catch-up and the rolling slice replay to
    // step - 1), and the join of the row updates at the step's end covers it.
    if ((rc = step_prologue(c, !pl.rows, s))) return rc;
    if ((rc = prepare_forward(c.T, c.W, 2, A.b, c.D, c.mimic, df, pl, A.timing_events + 2, A.timing_events,
                              A.timing_events + 8, A.timing_events + 12)))
        return rc;
    if (pl.rows && (rc = launch_step_begin(A.status, A.steps_applied, df.on ? df.hist : nullptr, df.on ? df.cap : 2,
                                           df.step, c.ad, pl.aux)))
        return rc;
    if (ws.ib_on && (rc = run_inbatch(c, s))) return rc;
    // score + loss (fwd + bwd seeds), + lambda * L_cal over cat[positives; negatives]
    // (training.py:805-820)
    if ((rc = launch_score_loss(bind_score(c), s))) return rc;
    if (ws.cal_on && (rc = launch_category_alignment(bind_cal_grads(c), s))) return rc;
    if (pl.rows) return rows_beside_mlp(c, pl, true);
    // one stream, or clipping (the table updates wait for the global norm)
    if ((rc = loss_finalize(c, s))) return rc;
    if ((rc = tower_backward(c.T, c.W, c.D, s, 2, A.timing_events + 6))) return rc;
    if (ws.clip_on && (rc = clip_coefficient(c, pl))) return rc;
    if ((rc = table_updates(c, c.T, c.W, 2, pl, false, A.timing_events, ws.clip_coef))) return rc;
    return dense_update(c.T, c.W, c.ad, A.status, s, ws.clip_coef);
}

// ---- the row-sharded step's phases (ttamm.h TTAMM_PHASE_*), in the order their bits execute -----
// ITEM_FWD / USER_FWD: the owner stages the requested local rows (range-checked) and their keys,
// contiguous, then the towers' forward — both in one grouped pass when the call asks for both
int phase_forward(Step& c, const StreamPlan& pl) {
    const ttamm_step_args& A = c.A;
    TowerWs& I = c.ws.item;
    const hipStream_t s = pl.s;
    const int ph = A.phase;
    int rc;
    if ((ph & TTAMM_PHASE_ITEM_FWD) && I.R > 0) {
        StageArgs st;
        std::memset(&st, 0, sizeof(st));
        st.status = A.status;
        st.seg[st.count++] = StageSeg{A.item_rows, I.idx_own, I.R, A.item.id.rows, A.item_rows_ld};
        st.seg[st.count++] = StageSeg{A.item_row_keys, c.ws.keys_own, I.R, INT64_MAX, A.item_rows_ld};
        if (compact_exchange(A)) {  // ... and their exchange units (requester groups as they arrived)
            st.unit_counts = A.exchange_counts + (int64_t)A.exchange_world * A.exchange_counts_ld;
            st.unit_ld = A.exchange_counts_ld;
            st.unit_groups = A.exchange_world;
            st.unit_n = I.R;
            st.unit_out = c.ws.own_units;
        }
        if ((rc = launch_stage_rows(st, s))) return rc;
    }
    const ttamm_tower* Ti[2] = {&A.item, nullptr};
    TowerWs* Wi[2] = {&I, nullptr};
    const int both = TTAMM_PHASE_ITEM_FWD | TTAMM_PHASE_USER_FWD;
    if ((ph & both) == both && I.R > 0)  // grouped: both towers' launches at once
        return prepare_forward(c.T, c.W, 2, A.b, c.D, c.mimic, c.df, pl, A.timing_events + 2, nullptr,
                               A.timing_events + 8);
    if (ph & TTAMM_PHASE_ITEM_FWD) {
        if (I.R > 0) {
            if ((rc = prepare_forward(Ti, Wi, 1, A.b, c.D, c.mimic, c.df, pl, A.timing_events + 2, nullptr,
                                      A.timing_events + 8)))
                return rc;
        } else if ((rc = tower_prepare(A.item, I, c.mimic, c.df, s))) {
            return rc;
        }
    }
    if (ph & TTAMM_PHASE_USER_FWD)
        return prepare_forward(c.T, c.W, 1, A.b, c.D, c.mimic, c.df, pl, nullptr, nullptr, A.timing_events + 8);
    return TTAMM_OK;
}

// no requests: this rank's item-tower gradient share is zero
int zero_item_grads(Step& c, hipStream_t s) {
    TowerWs& I = c.ws.item;
    const size_t n = tower_grad_floats(c.A.item);
    if (n) TTAMM_HIP(hipMemsetAsync(I.gw[0] ? I.gw[0] : I.ggw[0], 0, n * sizeof(float), s));
    return TTAMM_OK;
}

int run_phases(Step& c, const StreamPlan& pl) {
    const ttamm_step_args& A = c.A;
    StepWs& ws = c.ws;
    TowerWs& I = ws.item;
    const int D = c.D;
    const hipStream_t s = pl.s;
    const int ph = A.phase;
    const ttamm_tower* Ti[2] = {&A.item, nullptr};
    TowerWs* Wi[2] = {&I, nullptr};
    int rc;
    // ---- SAMPLE: the step's count and AdamW constants always with the prologue, on `s`
    if ((ph & TTAMM_PHASE_SAMPLE) && (rc = step_prologue(c, true, s))) return rc;
    // ---- ITEM_FWD / USER_FWD
    if ((ph & (TTAMM_PHASE_ITEM_FWD | TTAMM_PHASE_USER_FWD)) && (rc = phase_forward(c, pl))) return rc;
    // ---- INBATCH_SRC: this rank's positives' augmented rows for the all-gather
    if (ws.ib_on && (ph & TTAMM_PHASE_INBATCH_SRC)) {
        TTAMM_REQUIRE(A.item_fwd_in && A.inbatch_local, "INBATCH_SRC needs item_fwd_in and inbatch_local");
        const bool cx = compact_exchange(A);  // positives keep (t | a) in either layout
        if ((rc = launch_add_rows(A.item_fwd_in, cx ? D : 2 * D, c.mimic ? A.item_fwd_in + D : nullptr,
                                  cx ? D : 2 * D, c.B, D, A.inbatch_local, D, s, A.item_slot)))
            return rc;
    }
    // ---- INBATCH: the in-batch scores against every rank's positives
    if (ws.ib_on && (ph & TTAMM_PHASE_INBATCH)) {
        TTAMM_REQUIRE(A.inbatch_items && A.inbatch_dp_all, "INBATCH needs inbatch_items and inbatch_dp_all");
        if ((rc = run_inbatch(c, s))) return rc;
    }
    // ---- CAL_STATS / CAL_SCATTER: global per-category sums, then centered scatters
    if (ws.cal_on && (ph & TTAMM_PHASE_CAL_STATS) && (rc = launch_cal_local(bind_cal(c), s))) return rc;
    if (ws.cal_on && (ph & TTAMM_PHASE_CAL_SCATTER) && (rc = launch_cal_scatter(bind_cal(c), s))) return rc;
    // ---- USER / SCORE: score + loss (fwd + bwd seeds) against the received item rows; USER: the
    // user-side backward and table updates with it
    if (ph & (TTAMM_PHASE_USER | TTAMM_PHASE_SCORE)) {
        TTAMM_REQUIRE(!ws.ib_on || A.inbatch_dp, "sharded in-batch USER phase needs inbatch_dp");
        if ((rc = launch_score_loss(bind_score(c), s))) return rc;
        if (ws.cal_on && (rc = launch_cal_finish(bind_cal_grads(c), s))) return rc;
        if ((rc = loss_finalize(c, s))) return rc;
        if (ph & TTAMM_PHASE_USER) {
            if ((rc = tower_backward(c.T, c.W, D, s, 1))) return rc;
            if ((rc = table_updates(c, c.T, c.W, 1, pl, false, nullptr))) return rc;
        }
    }
    // ---- TOWERS_BWD (grouped): both towers' backward and table updates; with clipping the table
    // updates wait for the global norm (TABLES, after the caller's all-reduce of this rank's share)
    if ((ph & TTAMM_PHASE_TOWERS_BWD) && pl.rows) {
        if ((rc = rows_beside_mlp(c, pl, false))) return rc;
    } else if (ph & TTAMM_PHASE_TOWERS_BWD) {
        if ((rc = tower_backward(c.T, c.W, D, s, I.R > 0 ? 2 : 1, I.R > 0 ? A.timing_events + 6 : nullptr))) return rc;
        if (I.R == 0 && (rc = zero_item_grads(c, s))) return rc;
        if ((rc = ws.clip_on ? clip_table_share(c, pl) : table_updates(c, c.T, c.W, 2, pl, false, A.timing_events)))
            return rc;
    }
    // ---- TABLES (clipping): the table updates, scaled by clip_grad_norm_'s coefficient
    if ((ph & TTAMM_PHASE_TABLES) && ws.clip_on) {
        if ((rc = clip_coefficient_sharded(c, s))) return rc;
        if ((rc = table_updates(c, c.T, c.W, 2, pl, false, A.timing_events, ws.clip_coef))) return rc;
    }
    // ---- ITEM_BWD: the item-side backward and table updates on the owner
    if (ph & TTAMM_PHASE_ITEM_BWD) {
        if ((rc = I.R > 0 ? tower_backward(Ti, Wi, D, s, 1, A.timing_events + 6) : zero_item_grads(c, s))) return rc;
        if ((rc = table_updates(c, Ti, Wi, 1, pl, false, A.timing_events))) return rc;
    }
    if (ph & TTAMM_PHASE_DENSE) return dense_update(c.T, c.W, c.ad, A.status, s, ws.clip_on ? ws.clip_coef : nullptr);
    return TTAMM_OK;
}

}  // namespace

size_t train_step_workspace_size(const ttamm_step_args& A) {
    Arena ar{nullptr, 0, 0, true};
    StepWs ws;
    plan(ar, A, ws);
    return ar.off + 256;
}

int exchange_compact_supported(const ttamm_step_args& A) {
    if (!A.mimic_enabled || A.item.fusion != TTAMM_FUSION_GATED) return 0;
    const int D = out_dim(A.user);
    // the gate's choice as the step makes it, for the item tower alone (ITEM_FWD / ITEM_BWD) and for
    // both towers grouped: a gated tower has gate16 weight images exactly when plan() gives it some
    const ttamm_tower* T[2] = {&A.item, &A.user};
    bool has16[2];
    for (int k = 0; k < 2; ++k)
        has16[k] = T[k]->fusion == TTAMM_FUSION_GATED &&
                   gate16_supported(D, T[k]->gate[0].out_features, T[k]->matmul_bf16 ? 1 : 3);
    int hg, planes;
    return gate_choice(T, has16, 1, D, hg, planes) && gate_choice(T, has16, 2, D, hg, planes) ? 1 : 0;
}

int64_t dense_grad_floats(const ttamm_step_args& A) {
    return (int64_t)(tower_grad_floats(A.user) + tower_grad_floats(A.item));
}

int train_step(const ttamm_step_args& A, hipStream_t s) {
    Step c(A);
    int rc;
    if ((rc = bind_rows(c))) return rc;
    const StreamPlan pl = stream_plan(A, c.df, c.ws.clip_on, s);
    if (pl.rc) return pl.rc;
    return sharded(A) ? run_phases(c, pl) : run_single(c, pl);
}

int flush_tables(const ttamm_step_args& A, hipStream_t s) {
    Deferred df;
    int rc;
    if ((rc = deferred_of(A, df))) return rc;
    if (!df.on) return TTAMM_OK;
    const StreamPlan pl = stream_plan(A, df, A.hp.grad_clip_norm > 0.0, s);
    if (pl.rc) return pl.rc;
    ReplayArgs ra = replay_header(df, df.step, 1);
    for (const ttamm_tower* t : {&A.user, &A.item}) {
        const ttamm_table* tabs[2];
        const int n = dense_tables(*t, A.mimic_enabled != 0, tabs);
        for (int i = 0; i < n; ++i) {
            ReplaySeg g = replay_seg(*tabs[i]);
            g.row_lo = 0;
            g.row_hi = tabs[i]->rows;
            ra.seg[ra.count++] = g;
        }
    }
    if (!pl.aux) return launch_replay(ra, s);
    // With an aux stream the flush runs there (StreamPlan (c)): behind whatever wrote the tables —
    // the last step's row updates and slice on that stream already (tables_on_aux: the flush then
    // runs beside the main stream's tail of that step, the weight gradients, their reduce and the
    // dense update, which touch no table row; ~0.15 ms at C2), anything else on `s`, which the aux
    // stream waits for — and the main stream waits for it: the caller may read the tables, and the
    // next step gather them, without a host sync in between.
    if (!pl.tables_on_aux) {
        TTAMM_HIP(hipEventRecord(pl.ev[EV_TO_AUX], s));
        TTAMM_HIP(hipStreamWaitEvent(pl.aux, pl.ev[EV_TO_AUX], 0));
    }
    if ((rc = launch_replay(ra, pl.aux))) return rc;
    TTAMM_HIP(hipEventRecord(pl.ev[EV_FROM_AUX], pl.aux));
    TTAMM_HIP(hipStreamWaitEvent(s, pl.ev[EV_FROM_AUX], 0));
    return TTAMM_OK;
}

}  // namespace ttamm
