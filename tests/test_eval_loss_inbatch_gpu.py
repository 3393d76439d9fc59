"""The in-batch validation pass (ttamm.FusedEvalLoss(in_batch_negatives=True) /
ttamm.compute_loss(in_batch_negatives=True), ttamm_eval_loss_inbatch) on the MI355X vs the CPU
oracle.  The definition is ttamm's own (oracle/cpu_reference.py train_step(in_batch=True),
evaluated in eval mode; not reference behaviour): eval-mode towers and augment, S = U P^T over the
batch's positives with label 1 on the diagonal, the sampled negatives' logits with label 0, one
BCEWithLogits mean over all B (B + N) logits.

Tolerances are the project's eval-loss ones (tests/test_eval_loss_gpu.py): 1e-5 relative on the
loss, 1e-4 for bf16 towers; 2e-5 between the training step's reported bce and the validation
pass's on the same batch (each within 1e-5 of the definition)."""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import ttamm
from helpers import LOSS_WEIGHTS, Shape, clone_model, make_problem, rel_err
from oracle import cpu_reference as ref

pytestmark = pytest.mark.gpu

LOSS_TOL, BF16_LOSS_TOL = 1e-5, 1e-4


def oracle_inbatch_eval_batch(model, users, pos, neg, user_features, item_features) -> float:
    """One validation batch of the in-batch objective on the oracle model."""
    model.eval()
    mimic = model.adaptive_mimic
    with torch.no_grad():
        has_u = user_features is not None and user_features.numel() > 0
        has_i = item_features is not None and item_features.numel() > 0
        uf = user_features.index_select(0, users) if has_u else None
        pf = item_features.index_select(0, pos) if has_i else None
        u = ref.tower_forward(model.user_encoder, users, uf, training=False)
        p = ref.tower_forward(model.item_encoder, pos, pf, training=False)
        if mimic is not None:
            u = ref.gather_aug(mimic.user_augmented, users, u)[0]
            p = ref.gather_aug(mimic.item_augmented, pos, p)[0]
        ib = u @ p.T
        B = users.shape[0]
        neg_logits = ib.new_zeros((B, 0))
        if neg is not None and neg.numel() > 0:
            neg_flat = neg.reshape(-1)
            nf = item_features.index_select(0, neg_flat) if has_i else None
            n = ref.tower_forward(model.item_encoder, neg_flat, nf, training=False)
            if mimic is not None:
                n = ref.gather_aug(mimic.item_augmented, neg_flat, n)[0]
            n = n.view(B, -1, u.shape[-1])
            neg_logits = (u.unsqueeze(1) * n).sum(dim=-1)
        logits = torch.cat([ib.reshape(-1), neg_logits.reshape(-1)], dim=0)
        labels = torch.cat([torch.eye(B).reshape(-1), torch.zeros_like(neg_logits.reshape(-1))], dim=0)
        assert logits.numel() == B * (B + neg_logits.shape[1])
        loss = F.binary_cross_entropy_with_logits(logits, labels)
    return float(loss.item())


def _engine(prob, model, *, max_batch=None, seed=7, positives=True, in_batch=True):
    return ttamm.FusedEvalLoss(
        model, negatives_per_positive=prob.shape.N, positives=prob.positives if positives else None,
        user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
        max_batch=max_batch or prob.shape.B, seed=seed, in_batch_negatives=in_batch)


def _close(got: float, want: float, tol: float) -> bool:
    return abs(got - want) <= tol * abs(want)


CASES = {
    "tiny": Shape(),  # D = 8 (a multiple of 4); dropout 0.15 in the config must not apply
    "c2dims": Shape(U=300, I=2000, F=605, H=192, D=96, hidden_dims=(192,), B=67, N=5),
    "n0": Shape(N=0),
    "n1": Shape(U=64, I=512, F=20, H=32, D=32, hidden_dims=(32,), B=33, N=1),
    "d12-two-hidden": Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, gate_hidden=20, hidden_dims=(24, 16)),
    "nomimic": Shape(mimic=False),
    "sum": Shape(fusion="sum"),
    "max-norm": Shape(sparse=False, max_norm=0.05),
    "padding": Shape(padding_idx=5),
    "bf16-d128": Shape(U=300, I=2000, F=64, H=128, D=128, B=150, N=3, hidden_dims=(128,), matmul_dtype="bf16"),
}


def test_every_case_has_an_embedding_dim_the_kernel_takes():
    assert all(s.D % 4 == 0 and s.D <= 128 for s in CASES.values())
    assert {s.D for s in CASES.values()} >= {8, 12, 32, 96, 128}


@pytest.mark.parametrize("case", list(CASES))
def test_loss_matches_oracle_and_nothing_else_moves(case):
    from gpu_helpers import ttamm_model_from

    shape = CASES[case]
    prob = make_problem(shape, steps=1)
    users, pos, neg, _, _ = prob.batches[0]
    om = clone_model(prob.model)
    want = oracle_inbatch_eval_batch(om, users, pos, neg, prob.user_features, prob.item_features)

    model = ttamm_model_from(prob).eval()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = _engine(prob, model)
    eng.step(users.cuda(), pos.cuda(), neg.cuda() if shape.N else None)
    last = eng.last_loss()
    got = eng.finish()
    bf16 = shape.matmul_dtype == "bf16"
    print(f"\n{case}: loss {got:.8f} oracle {want:.8f} rel {abs(got - want) / abs(want):.2e}")
    assert last == got  # one batch: the pass's weighted mean is that batch's BCE
    assert _close(got, want, BF16_LOSS_TOL if bf16 else LOSS_TOL)
    assert eng.loss_out.tolist() == [last, last, 0.0, 0.0, 0.0]

    after = model.state_dict()
    if shape.max_norm is None:
        for k, v in before.items():
            assert torch.equal(after[k], v), k
    else:
        # nn.Embedding(max_norm) renorms the looked-up rows in eval mode too, as in the oracle
        init = prob.model.state_dict()
        for k, v in before.items():
            if k.endswith("embedding.weight"):
                o = om.state_dict()[k]
                moved_o = (o != init[k]).any(dim=1)
                moved_t = (after[k].cpu() != init[k]).any(dim=1)
                assert moved_o.any() and torch.equal(moved_o, moved_t), k
                assert rel_err(after[k], o) <= 1e-6, k
            else:
                assert torch.equal(after[k], v), k
    assert all(p.grad is None for p in model.parameters())
    assert not model.training


@pytest.mark.parametrize("shape", [
    Shape(dropout=0.0),
    Shape(dropout=0.0, N=0),
    Shape(U=300, I=2000, F=64, H=96, D=96, B=150, N=2, hidden_dims=(96,), dropout=0.0),
], ids=["tiny", "n0", "d96"])
def test_validation_bce_is_the_training_steps_bce_on_the_same_batch(shape):
    """Dropout-free towers: the training step's forward is the eval forward, and the bce it
    reports is taken before its update."""
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    prob = make_problem(shape, steps=1)
    users, pos, neg, um, im = prob.batches[0]
    assert all(bool(m.all()) for m in um + im)  # keep masks of all ones
    tm = ttamm_model_from(prob)
    tr = ttamm.FusedTrainStep(tm, ttamm_optimizers(tm), negatives_per_positive=shape.N, positives=prob.positives,
                              user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                              loss_weights=LOSS_WEIGHTS, max_batch=shape.B, in_batch_negatives=True)
    tr.step(users.cuda(), pos.cuda(), neg.cuda().reshape(-1) if shape.N else None,
            keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})
    train_bce = tr.last_losses()["bce"]
    tr.finish()

    eng = _engine(prob, ttamm_model_from(prob))  # a fresh copy of the model
    eng.step(users.cuda(), pos.cuda(), neg.cuda() if shape.N else None)
    val_bce = eng.finish()
    print(f"\ntraining bce {train_bce:.8f} validation bce {val_bce:.8f} rel {abs(train_bce - val_bce) / val_bce:.2e}")
    assert _close(train_bce, val_bce, 2e-5)


def test_multi_batch_pass_through_compute_loss():
    from gpu_helpers import ttamm_model_from

    prob = make_problem(Shape(), steps=3)
    sizes = (32, 32, 13)  # the last batch ragged
    batches = [(u[:s], p[:s], n[:s]) for (u, p, n, _, _), s in zip(prob.batches, sizes)]
    om = clone_model(prob.model)
    per = [oracle_inbatch_eval_batch(om, u, p, n, prob.user_features, prob.item_features) for u, p, n in batches]
    want = sum(l * s for l, s in zip(per, sizes)) / sum(sizes)  # weighted by positives

    model = ttamm_model_from(prob)
    assert model.training
    kw = dict(criterion=nn.BCEWithLogitsLoss(), negatives_per_positive=prob.shape.N, num_items=prob.shape.I,
              user_positive_items=prob.positives, user_features=prob.user_features.cuda(),
              item_features=prob.item_features.cuda(), device=torch.device("cuda"), in_batch_negatives=True)
    pairs = [(u, p) for u, p, _ in batches]
    got = ttamm.compute_loss(model, pairs, batch_hook=lambda step, users, pos: (batches[step][2], None), **kw)
    print(f"\ncompute_loss {got:.8f} oracle {want:.8f}")
    assert _close(got, want, LOSS_TOL), (got, want)
    assert not model.training

    # on-device sampling: one seed, the same bits; another seed, other negatives
    a = ttamm.compute_loss(model, pairs, seed=11, **kw)
    b = ttamm.compute_loss(model, pairs, seed=11, **kw)
    c = ttamm.compute_loss(model, pairs, seed=12, **kw)
    assert a == b and a != c

    # N = 0: a hook's negatives are ignored, user_positive_items may be None
    kw0 = dict(kw, negatives_per_positive=0, user_positive_items=None)
    per0 = [oracle_inbatch_eval_batch(om, u, p, None, prob.user_features, prob.item_features) for u, p, _ in batches]
    want0 = sum(l * s for l, s in zip(per0, sizes)) / sum(sizes)
    got0 = ttamm.compute_loss(model, pairs, batch_hook=lambda step, users, pos: batches[step][2], **kw0)
    assert _close(got0, want0, LOSS_TOL), (got0, want0)
    assert ttamm.compute_loss(model, [], **kw) == 0.0


def test_sampled_negatives_are_the_plain_passes_draws_and_are_scored():
    from gpu_helpers import ttamm_model_from

    shape = Shape(I=256, N=5)
    prob = make_problem(shape, steps=2, positives_per_user=4)
    model = ttamm_model_from(prob)
    plain = _engine(prob, model, seed=11, in_batch=False)
    ib = _engine(prob, model, seed=11)
    om = clone_model(prob.model)
    for k, (users, pos, _, _, _) in enumerate(prob.batches):  # counters 0 and 1
        plain.step(users.cuda(), pos.cuda())
        want_neg = plain.neg_buffer[: shape.B * shape.N].clone()
        ib.step(users.cuda(), pos.cuda())
        neg = ib.neg_buffer[: shape.B * shape.N].clone()
        assert torch.equal(neg, want_neg), k
        want = oracle_inbatch_eval_batch(om, users, pos, neg.cpu().view(shape.B, shape.N), prob.user_features,
                                         prob.item_features)
        assert _close(ib.last_loss(), want, LOSS_TOL), (k, ib.last_loss(), want)
    plain.finish()
    ib.finish()


def test_errors_surface_at_finish_and_bad_arguments_raise():
    from gpu_helpers import ttamm_model_from

    prob = make_problem(Shape(), steps=3)
    model = ttamm_model_from(prob)
    eng = _engine(prob, model)
    for k, (u, p, n, _, _) in enumerate(prob.batches):
        u = u.clone()
        if k == 1:
            u[5] = prob.shape.U  # == user rows: read as row 0 on the device, reported by the status word
        eng.step(u.cuda(), p.cuda(), n.cuda())
    torch.cuda.synchronize()
    u0, p0, n0, _, _ = prob.batches[0]
    first = oracle_inbatch_eval_batch(clone_model(prob.model), u0, p0, n0, prob.user_features, prob.item_features)
    total, count = eng.loss_accum.tolist()
    assert count == prob.shape.B  # exactly the first batch: the bad one and the one after it wrote nothing
    assert _close(total / count, first, LOSS_TOL)
    with pytest.raises(IndexError, match="index out of range in self"):
        eng.finish()
    assert eng.finish() == 0.0  # the raise left the engine clean

    u, p, n = u0.cuda(), p0.cuda(), n0.cuda()
    logits = torch.empty(prob.shape.B * (1 + prob.shape.N), device="cuda")
    with pytest.raises(ValueError, match="logits_out is not available in in-batch mode"):
        eng.step(u, p, n, logits_out=logits)
    with pytest.raises(ValueError, match=r"negatives must be int64 \[batch, negatives_per_positive\]"):
        eng.step(u, p, n.reshape(-1)[:-1])
    with pytest.raises(ValueError, match="positives are required to sample negatives"):
        _engine(prob, model, positives=False).step(u, p)
    assert eng.finish() == 0.0  # nothing was enqueued by the rejected calls

    bad = make_problem(Shape(U=20, I=30, F=6, H=10, D=10, hidden_dims=(10,), gate_hidden=10, B=8, N=2), steps=1)
    with pytest.raises(ValueError, match="embedding dim must be a multiple of 4, <= 128"):
        _engine(bad, ttamm_model_from(bad))
