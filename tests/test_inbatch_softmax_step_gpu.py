"""The in-batch softmax objective in the fused step and the validation pass
(ttamm_step_args.in_batch_loss / in_batch_inv_temperature; FusedTrainStep / FusedEvalLoss /
compute_loss ``in_batch_loss="softmax"``) against tests/softmax_reference.train_step_softmax: the
oracle's train_step with the retrieval term F.cross_entropy((u @ p^T) / t, arange(B)).

Problems as in tests/test_inbatch_gpu.py (tests/helpers.py: gated towers, mimic on), N = 0.  Same
tolerances as there: loss and every gradient 1e-5 norm-wise relative, three real steps as
test_inbatch_three_steps_match_oracle.

The one-step reference is the helper on a float64 copy of the model.  In float32 the helper is
itself up to 1.7e-5 from that on the two last-layer bias gradients (CANCELLING below), more than
the bound it is to judge; its float32 figures are printed next to the asserted ones."""

from __future__ import annotations

import functools

import pytest
import torch
from torch import nn

import ttamm
from helpers import LOSS_WEIGHTS, Shape, clone_model, make_problem, named_optimizer_state, rel_err, set_lr
from oracle import cpu_reference as ref
from softmax_reference import train_step_softmax

pytestmark = pytest.mark.gpu

TOL = 1e-5

SHAPES = [
    Shape(N=0),
    Shape(U=400, I=2000, F=64, H=96, D=96, B=300, N=0, hidden_dims=(96,)),  # three row blocks, five splits
]
IDS = ["tiny", "d96-b300"]


def _run_oracle(prob, temperature, *, lr=1e-3, betas=(0.9, 0.999), dtype=torch.float32):
    """train_step_softmax over the problem's batches on a copy of the model in dtype."""
    model = clone_model(prob.model).to(dtype)
    opts = ref.build_optimizers(model, lr=lr or 1e-3, betas=betas, weight_decay=0.01)
    set_lr(opts, lr)
    res = []
    for (users, pos, _, um, im) in prob.batches:
        res.append(train_step_softmax(model, opts, users, pos, temperature=temperature,
                                      user_features=prob.user_features.to(dtype),
                                      item_features=prob.item_features.to(dtype),
                                      loss_weights=LOSS_WEIGHTS, user_keep_masks=um, item_keep_masks=im))
    return model, opts, res


def _run_ttamm(prob, *, lr=1e-3, betas=(0.9, 0.999), **objective):
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    model = ttamm_model_from(prob)
    opts = ttamm_optimizers(model, lr=lr, betas=betas)
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=0, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, in_batch_negatives=True, **objective)
    losses = []
    for (users, pos, _, um, im) in prob.batches:
        eng.step(users.cuda(), pos.cuda(), None,
                 keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})
        losses.append(eng.last_losses())
    eng.finish()
    return model, opts, losses


# The last Linear's bias of each feature encoder: its gradient is a sum over the batch of rows that
# cancel under softmax (every row of dS sums to 0, so the retrieval part of sum_j dP_j vanishes and
# sum_b dU_b nearly does), which leaves a small difference of large terms.
CANCELLING = ("user_encoder.feature_encoder.network.3.bias", "item_encoder.feature_encoder.network.3.bias")


@functools.lru_cache(maxsize=None)
def _one_step(shape_id: str, temperature: float):
    """(float64 helper losses, ttamm losses, {tensor: (ttamm vs float64 helper: the one asserted,
    ttamm vs float32 helper, float32 helper vs float64 helper)}) of one step at lr = 0,
    betas = (0, .999): exp_avg is then the gradient."""
    prob = make_problem(SHAPES[IDS.index(shape_id)], steps=1)
    kw = dict(lr=0.0, betas=(0.0, 0.999))
    o64, oo64, ores = _run_oracle(prob, temperature, dtype=torch.float64, **kw)
    o32, oo32, _ = _run_oracle(prob, temperature, **kw)  # for the record only
    tm, to, tres = _run_ttamm(prob, in_batch_loss="softmax", temperature=temperature, **kw)
    g64 = {n: st["exp_avg"] for n, st in named_optimizer_state(o64, oo64).items()}
    g32 = {n: st["exp_avg"] for n, st in named_optimizer_state(o32, oo32).items()}
    tg = {n: st["exp_avg"] for n, st in named_optimizer_state(tm, to).items()}
    assert set(g64) == set(tg)
    errs = {n: (rel_err(tg[n], g64[n]), rel_err(tg[n], g32[n]), rel_err(g32[n], g64[n])) for n in g64}
    return ores[0], tres[0], errs


def _report(errs, names):
    for n in sorted(names, key=lambda n: -errs[n][0])[:4]:
        e = errs[n]
        print(f"\n{n}: ttamm vs float64 helper {e[0]:.2e}; vs float32 helper {e[1]:.2e}; float32 helper vs float64 {e[2]:.2e}", end="")


@pytest.mark.parametrize("temperature", [1.0, 0.25])
@pytest.mark.parametrize("shape_id", IDS)
def test_softmax_step_losses_and_gradients_match_oracle(shape_id, temperature):
    """The four losses and every gradient-bearing tensor but the two of CANCELLING (next test)."""
    o, t, errs = _one_step(shape_id, temperature)
    for key in ("total", "bce", "mimic_user", "mimic_item"):  # "bce": the retrieval slot, here the softmax mean
        assert abs(t[key] - getattr(o, key)) <= TOL * abs(getattr(o, key)), (key, t[key], getattr(o, key))
    names = [n for n in errs if n not in CANCELLING]
    assert len(names) == len(errs) - 2
    _report(errs, names)
    bad = {n: f"{errs[n][0]:.3e}" for n in names if errs[n][0] > TOL}
    assert not bad, f"rel err above {TOL}: {bad}"


@pytest.mark.parametrize("temperature", [1.0, 0.25])
@pytest.mark.parametrize("shape_id", IDS)
def test_softmax_step_last_layer_bias_gradients_match_oracle(shape_id, temperature):
    """The same check on the two CANCELLING tensors.  Measured on the MI355X (max|a - b| / max|b|):

        case            tensor     ttamm vs float64   float32 helper vs float64   ttamm vs float32 helper
        tiny, t = 1     item bias  7.06e-06           1.66e-05                    1.78e-05
                        user bias  2.00e-06           4.23e-06                    6.22e-06
        tiny, t = .25   item bias  6.94e-06           1.07e-05                    5.09e-06
                        user bias  4.41e-07           1.18e-06                    1.62e-06
        d96-b300, t = 1 item bias  7.47e-06           7.34e-06                    1.19e-05
                        user bias  3.00e-06           2.19e-06                    3.49e-06
        d96-b300, .25   item bias  6.46e-06           7.76e-06                    9.68e-06
                        user bias  5.98e-07           5.66e-07                    7.70e-07

    Every other tensor is within 2e-6.  The batch sum cancels to a few percent of its terms, which
    multiplies any float32 rounding of the rows of dS: what decides these two is how far a row of
    p is from summing to 1.  With the row normaliser carried as one float lse the kernel was at
    1.3e-5 to 5.0e-5 here; carried as (row maximum, 1 / sum) it is where float32 torch is."""
    o, t, errs = _one_step(shape_id, temperature)
    _report(errs, CANCELLING)
    bad = {n: f"{errs[n][0]:.3e}" for n in CANCELLING if errs[n][0] > TOL}
    assert not bad, f"rel err above {TOL}: {bad}"


def test_softmax_three_steps_match_oracle():
    prob = make_problem(Shape(N=0), steps=3)
    om, oo, ores = _run_oracle(prob, 0.25)
    tm, to, tres = _run_ttamm(prob, in_batch_loss="softmax", temperature=0.25)
    for o, t in zip(ores, tres):
        assert abs(t["total"] - o.total) <= 1e-5 * abs(o.total)
    osd, tsd = om.state_dict(), tm.state_dict()
    for n in osd:
        d = (tsd[n].cpu() - osd[n]).abs().max().item()
        assert d <= 1e-3 * 1e-3 * 50, f"{n}: max abs diff {d:.3e}"


def test_validation_pass_matches_the_helper_and_the_training_step():
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    t = 0.25
    prob = make_problem(Shape(N=0, dropout=0.0), steps=2)
    sizes = (32, 13)  # the second batch short
    batches = [(u[:s], p[:s]) for (u, p, _, _, _), s in zip(prob.batches, sizes)]
    om = clone_model(prob.model)
    per = [train_step_softmax(om, [], u, p, temperature=t, user_features=prob.user_features,
                              item_features=prob.item_features, train=False).bce for u, p in batches]
    want = sum(l * s for l, s in zip(per, sizes)) / sum(sizes)  # weighted by positives, as _compute_loss

    model = ttamm_model_from(prob)
    kw = dict(criterion=nn.BCEWithLogitsLoss(), negatives_per_positive=0, num_items=prob.shape.I,
              user_positive_items=None, user_features=prob.user_features.cuda(),
              item_features=prob.item_features.cuda(), device=torch.device("cuda"), in_batch_negatives=True)
    got = ttamm.compute_loss(model, batches, in_batch_loss="softmax", temperature=t, **kw)
    print(f"\ncompute_loss {got:.8f} helper {want:.8f}")
    assert abs(got - want) <= TOL * abs(want), (got, want)
    assert got == ttamm.compute_loss(model, batches, in_batch_loss="softmax", temperature=t, **kw)
    assert not model.training
    bce = ttamm.compute_loss(model, batches, **kw)  # the default objective is another number
    assert abs(bce - got) > 1e-3 * abs(got)

    # dropout-free towers: the training step's forward is the eval forward, and the loss it reports
    # is taken before its update
    users, pos, _, um, im = prob.batches[0]
    tm = ttamm_model_from(prob)
    tr = ttamm.FusedTrainStep(tm, ttamm_optimizers(tm, lr=0.0, betas=(0.0, 0.999)), negatives_per_positive=0,
                              positives=prob.positives, user_features=prob.user_features.cuda(),
                              item_features=prob.item_features.cuda(), loss_weights=LOSS_WEIGHTS,
                              max_batch=prob.shape.B, in_batch_negatives=True, in_batch_loss="softmax", temperature=t)
    tr.step(users.cuda(), pos.cuda(), None,
            keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})
    train_loss = tr.last_losses()["bce"]
    tr.finish()
    val = ttamm.compute_loss(ttamm_model_from(prob), [(users, pos)], in_batch_loss="softmax", temperature=t, **kw)
    print(f"training softmax loss {train_loss:.8f} validation {val:.8f}")
    assert abs(train_loss - val) <= 2e-5 * abs(val)


def test_sharded_step_refuses_softmax():
    from gpu_helpers import ttamm_model_from, ttamm_optimizers
    from ttamm.sharded import ShardedTrainStep

    prob = make_problem(Shape(N=0), steps=1)
    model = ttamm_model_from(prob)
    with pytest.raises(NotImplementedError, match="in_batch_loss='softmax' is not built for the row-sharded step"):
        ShardedTrainStep(model, ttamm_optimizers(model), world_size=1, rank=0, num_items=prob.shape.I,
                         negatives_per_positive=0, positives=prob.positives,
                         user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                         loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, in_batch_negatives=True,
                         in_batch_loss="softmax")


def test_default_objective_is_bit_identical_to_omitting_the_keyword():
    prob = make_problem(Shape(N=0), steps=2)
    am, ao, ares = _run_ttamm(prob)
    bm, bo, bres = _run_ttamm(prob, in_batch_loss="bce")
    cm, co, cres = _run_ttamm(prob, in_batch_loss="bce", temperature=0.25)  # the temperature is softmax's alone
    assert ares == bres == cres
    for other in (bm, cm):
        for (n, a), (_, b) in zip(am.state_dict().items(), other.state_dict().items()):
            assert torch.equal(a, b), n
