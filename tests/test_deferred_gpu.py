"""Deferred exact AdamW(g = 0) on the dense-group tables (ttamm.h ttamm_table.last_step)
against the eager per-step sweep: after any number of steps and a flush, every parameter and
every optimizer moment is BIT-identical (the deferred path replays the same fp32 operations
with the same per-step constants).  Covered: rows lagging up to replay_slices steps, the
history ring wrapping, a learning-rate change mid-run (per-step constants), a mid-run flush,
a dense-optimized ID table, the C2 shapes, and torch.optim.SGD in the dense group."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

import ttamm
from helpers import LOSS_WEIGHTS, Shape, make_problem

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _engine(prob, *, deferred: bool, slices: int, sparse: bool = True, overlap: bool = True, math: str = "fast",
            aux_cus=None, sgd: dict | None = None, gradient_clip_norm: float | None = None, coupled: bool = False):
    from gpu_helpers import ttamm_model_from

    model = ttamm_model_from(prob)
    dense, sp = ttamm._collect_parameter_groups(model)
    if not sparse:  # every table in the AdamW group (the reference's sparse=False configuration)
        dense, sp = dense + sp, []
    if sgd is not None:  # optimizer: sgd (training.py:1324-1330)
        opts = [torch.optim.SGD(dense, lr=1e-3, weight_decay=0.01, **sgd)]
    else:  # coupled: torch.optim.Adam with L2 weight decay (training.py:1311, test_optimizers_gpu.py)
        opts = [(torch.optim.Adam if coupled else torch.optim.AdamW)(dense, lr=1e-3, weight_decay=0.01)]
    if sp:
        opts.append(torch.optim.SparseAdam(sp, lr=1e-3))
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=prob.shape.N, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, seed=11,
                               deferred_adamw=deferred, replay_slices=slices, overlap=overlap,
                               table_adamw_math=math, aux_cus=aux_cus, gradient_clip_norm=gradient_clip_norm)
    return model, opts, eng


def _state(model, opts):
    out = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for i, o in enumerate(opts):
        for j, (p, st) in enumerate(o.state.items()):
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"opt{i}.{j}.{k}"] = v.detach().clone()
    return out


def _batches(prob, steps):
    gen = torch.Generator().manual_seed(3)
    for _ in range(steps):
        users = torch.randint(0, prob.shape.U, (prob.shape.B,), generator=gen)
        pos = torch.tensor([sorted(prob.positives[int(u)])[0] for u in users], dtype=torch.long)
        yield users.cuda(), pos.cuda()


def _run(prob, steps, *, deferred, slices, sparse=True, flush_at=None, lr_change_at=None, overlap=True, math="fast",
         aux_cus=None, sgd=None, gradient_clip_norm=None, coupled=False):
    model, opts, eng = _engine(prob, deferred=deferred, slices=slices, sparse=sparse, overlap=overlap, math=math,
                               aux_cus=aux_cus, sgd=sgd, gradient_clip_norm=gradient_clip_norm, coupled=coupled)
    losses = []
    for k, (users, pos) in enumerate(_batches(prob, steps)):
        if lr_change_at is not None and k == lr_change_at:
            for o in opts:
                for g in o.param_groups:
                    g["lr"] = 3e-3
        eng.step(users, pos)
        losses.append(eng.last_losses()["total"])
        if flush_at is not None and k == flush_at:
            eng.flush()
    eng.finish()
    return _state(model, opts), losses


@pytest.mark.parametrize("math", ["fast", "exact"])
@pytest.mark.parametrize("slices,steps,sparse", [(3, 13, True), (1, 4, True), (5, 17, False)])
def test_deferred_equals_eager_bitwise(slices, steps, sparse, math):
    prob = make_problem(Shape(), seed=21)
    eager, le = _run(prob, steps, deferred=False, slices=slices, sparse=sparse, lr_change_at=steps // 2, math=math)
    lazy, ll = _run(prob, steps, deferred=True, slices=slices, sparse=sparse, lr_change_at=steps // 2,
                    flush_at=steps // 3, math=math)
    assert le == ll
    assert eager.keys() == lazy.keys()
    for k in eager:
        assert torch.equal(eager[k], lazy[k]), k


@pytest.mark.parametrize("sgd", [dict(momentum=0.9), dict(momentum=0.9, nesterov=True),
                                 dict(momentum=0.8, dampening=0.1), dict(momentum=0.0)],
                         ids=["momentum", "nesterov", "dampening", "no-momentum"])
@pytest.mark.parametrize("slices,steps,sparse", [(3, 13, True), (5, 17, False)])
def test_deferred_sgd_equals_eager_bitwise(sgd, slices, steps, sparse):
    """optimizer: sgd (training.py:1324-1330): the g = 0 steps of untouched table rows (weight decay
    through the momentum buffer) replayed from the history ring equal the eager per-step sweep bit
    for bit, with lagging rows, a mid-run lr change, a mid-run flush and (dampening) the first
    step's buf = grad."""
    prob = make_problem(Shape(), seed=21)
    eager, le = _run(prob, steps, deferred=False, slices=slices, sparse=sparse, lr_change_at=steps // 2, sgd=sgd)
    lazy, ll = _run(prob, steps, deferred=True, slices=slices, sparse=sparse, lr_change_at=steps // 2,
                    flush_at=steps // 3, sgd=sgd)
    assert le == ll
    assert eager.keys() == lazy.keys()
    for k in eager:
        assert torch.equal(eager[k], lazy[k]), k


@pytest.mark.parametrize("deferred,sparse", [(True, True), (False, True), (True, False)])
def test_aux_stream_overlap_bitwise(deferred, sparse):
    """The index-only prologue on the aux stream (ttamm_step_args.aux_stream) changes no bit:
    same losses, parameters and moments as the one-stream step."""
    prob = make_problem(Shape(), seed=5)
    one, l1 = _run(prob, 9, deferred=deferred, slices=3, sparse=sparse, overlap=False)
    two, l2 = _run(prob, 9, deferred=deferred, slices=3, sparse=sparse, overlap=True)
    # the aux stream restricted to 16 CUs (ttamm_stream_create_cu_limited)
    three, l3 = _run(prob, 9, deferred=deferred, slices=3, sparse=sparse, overlap=True, aux_cus=16)
    assert l1 == l2 == l3
    for k in one:
        assert torch.equal(one[k], two[k]), k
        assert torch.equal(one[k], three[k]), k


_EAGER_DENSE_ID: dict = {}


def _eager_dense_id(clip):
    """The eager one-stream run of the flush tests' problem (dense ID tables), once per clip norm."""
    if clip not in _EAGER_DENSE_ID:
        prob = make_problem(Shape(), seed=5)
        _EAGER_DENSE_ID[clip], _ = _run(prob, 9, deferred=False, slices=3, sparse=False, overlap=False,
                                        gradient_clip_norm=clip)
    return _EAGER_DENSE_ID[clip]


@pytest.mark.parametrize("clip,aux_cus", [(1.0, None), (None, None), (1.0, 16)],
                         ids=["clip", "dense-id", "clip-aux-cus"])
def test_flush_without_sync_is_ordered(clip, aux_cus):
    """flush() right behind the last step, no host sync in between: the flush's replay (on the aux
    stream when there is one) must follow that step's table updates on the caller's stream, and
    the caller's stream the replay.  The cases are the ones whose row updates run on the caller's
    stream although an aux stream exists: gradient clipping (the updates wait for the global norm)
    and deferred dense ID tables (no fork); with aux_cus the flush itself runs on the caller's
    stream.  Clipping needs dense ID tables (FusedTrainStep raises NotImplementedError for sparse
    ones, as torch's clip_grad_norm_ does), so every case has them.  The snapshot is taken on the
    current stream right after the flush (the clones are stream-ordered behind it), before any
    synchronisation; it equals the eager one-stream run bit for bit.  (The optimizers' `step`
    counters are written by finish() and are not part of the snapshot.)"""
    prob = make_problem(Shape(), seed=5)
    model, opts, eng = _engine(prob, deferred=True, slices=3, sparse=False, overlap=True, aux_cus=aux_cus,
                               gradient_clip_norm=clip)
    for users, pos in _batches(prob, 9):
        eng.step(users, pos)
    eng.flush()
    snap = _state(model, opts)
    eng.finish()
    eager = _eager_dense_id(clip)
    assert snap.keys() == eager.keys()
    for k in eager:
        if not k.endswith(".step"):
            assert torch.equal(snap[k], eager[k]), k


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_steps_applied_visible_after_stream_sync(deferred):
    """Gradient clipping with an aux stream: after a synchronise of the caller's stream alone every
    enqueued step is counted in steps_applied (INTEGRATION.md "Streams"; _status_error reads it
    there).  Eager is the case in which the count used to be published on the aux stream although
    clipping keeps the step's closing join away; deferred dense ID tables run on one stream."""
    prob = make_problem(Shape(), seed=5)
    model, opts, eng = _engine(prob, deferred=deferred, slices=3, sparse=False, overlap=True, gradient_clip_norm=1.0)
    for users, pos in _batches(prob, 5):
        eng.step(users, pos)
    torch.cuda.current_stream().synchronize()
    applied, status = int(eng.steps_applied.item()), int(eng.status.item())
    eng.finish()
    assert applied == 5
    assert status == 0


def test_deferred_c2_equals_eager():
    """C2 shapes, 4 steps, default slices: bit-identical tables and moments after flush."""
    sys.path.insert(0, str(ROOT))
    import bench

    c2 = bench.CONFIGS["c2"]
    sums = []
    for deferred in (False, True):
        w = bench.Workload(c2, torch.device("cuda"), seed=8, deferred=deferred)
        for _ in range(4):
            w.engine.step(*w.batch())
        w.engine.finish()
        mm = w.model.adaptive_mimic
        st = w.opts[0].state[mm.item_augmented.weight]
        sums.append([mm.item_augmented.weight.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                     [float(p.detach().double().sum()) for p in w.model.parameters()]])
        del w
        torch.cuda.empty_cache()
    for a, b in zip(sums[0][:3], sums[1][:3]):
        assert torch.equal(a, b)
    assert sums[0][3] == sums[1][3]


def test_deferred_c2_fast_overlap_repeatable():
    """The bench's configuration (C2, fast g = 0 arithmetic, replay slices on the aux stream beside
    the MLP GEMMs) run twice from the same seed: bit-identical tables and moments (the regression
    check for the packed-operand hazard of round 4, tools/diag/deferred_c2.py: a race or hazard that
    comes back shows as run-to-run differences even if tools/check_pk_operands.py finds nothing)."""
    sys.path.insert(0, str(ROOT))
    import bench

    c2 = bench.CONFIGS["c2"]
    runs = []
    for _ in range(2):
        w = bench.Workload(c2, torch.device("cuda"), seed=11, deferred=True, table_math="fast")
        for _ in range(5):
            w.engine.step(*w.batch())
        w.engine.finish()
        mm = w.model.adaptive_mimic
        st = w.opts[0].state[mm.item_augmented.weight]
        su = w.opts[0].state[mm.user_augmented.weight]
        runs.append([mm.item_augmented.weight.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                     mm.user_augmented.weight.detach().clone(), su["exp_avg"].clone(), su["exp_avg_sq"].clone()])
        del w
        torch.cuda.empty_cache()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_fast_g0_math_close_to_exact():
    """table_adamw_math="fast" (v_sqrt / v_rcp for the g = 0 updates) against the IEEE path over
    17 steps with lagging rows: every parameter and moment within 1e-6 of the tensor's largest
    magnitude (each g = 0 update term within a few ulp; the moments of g = 0 rows do not depend
    on the arithmetic, the rest differ only through the parameters the forward reads)."""
    prob = make_problem(Shape(), seed=21)
    fast, lf = _run(prob, 17, deferred=True, slices=5, math="fast")
    exact, lx = _run(prob, 17, deferred=True, slices=5, math="exact")
    for a, b in zip(lf, lx):
        assert abs(a - b) <= 1e-6 * abs(b)
    for k in exact:
        d = (fast[k].double() - exact[k].double()).abs().max().item()
        scale = exact[k].double().abs().max().item()
        assert d <= 1e-6 * max(scale, 1e-30), (k, d, scale)


def test_fast_g0_drift_bounded_over_many_steps():
    """The fast g = 0 arithmetic over a long horizon: 150 steps on a 4096-item table that a
    32-row batch mostly misses, so most item rows take 100+ consecutive g = 0 updates (each a few
    ulp from torch's IEEE step).  Bound: every parameter within 2 ulp of its magnitude per step
    of the IEEE path (fast vs exact), and far below the parameters' own movement; the moments are
    the same operations in both modes (only the parameters the forward reads differ)."""
    steps = 150
    prob = make_problem(Shape(U=64, I=4096, B=32, N=5), seed=5)
    init = {k: v.detach().clone() for k, v in prob.model.state_dict().items()}
    fast, _ = _run(prob, steps, deferred=True, slices=8, math="fast")
    exact, _ = _run(prob, steps, deferred=True, slices=8, math="exact")
    name = "adaptive_mimic.item_augmented.weight"
    f, e = fast[name].double(), exact[name].double()
    err = (f - e).abs().max().item()
    ulp = torch.finfo(torch.float32).eps * e.abs().max().item()
    moved = (e.cpu() - init[name].double()).abs().max().item()
    print(f"\nfast vs exact after {steps} steps: max |diff| {err:.3e} = {err / ulp:.1f} ulp(max|p|); "
          f"max movement {moved:.3e}")
    assert err <= 2 * steps * ulp, (err, ulp)
    assert err <= 1e-3 * moved, (err, moved)
