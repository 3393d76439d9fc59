"""Fused validation loss (ttamm.FusedEvalLoss / ttamm.compute_loss, ttamm_eval_loss) on the MI355X
vs the CPU oracle's restatement of `_compute_loss`'s batch body (training.py:854-910): eval-mode
towers, mimic augment, dot-product scores, BCEWithLogits mean — same parameters, same negatives.

Tolerances are the project's: fp32 towers 1e-5 relative on the loss and 1e-5 norm-wise relative
(helpers.rel_err) on the logits; bf16 towers 1e-4 on the loss and 2e-3 on the logits
(tests/test_step_parity_gpu.py GRAD_TOL / BF16_TOL)."""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import ttamm
from helpers import LOSS_WEIGHTS, Shape, clone_model, make_problem, rel_err, run_oracle
from oracle import cpu_reference as ref

pytestmark = pytest.mark.gpu

LOSS_TOL, LOGIT_TOL = 1e-5, 1e-5
BF16_LOSS_TOL, BF16_LOGIT_TOL = 1e-4, 2e-3


def oracle_eval_batch(model, users, pos, neg, user_features, item_features):
    """One iteration of `_compute_loss` (training.py:854-908) on the oracle model: (loss, logits)."""
    model.eval()
    mimic = model.adaptive_mimic
    with torch.no_grad():
        neg_flat = neg.reshape(-1)
        has_u = user_features is not None and user_features.numel() > 0
        has_i = item_features is not None and item_features.numel() > 0
        uf = user_features.index_select(0, users) if has_u else None
        pf = item_features.index_select(0, pos) if has_i else None
        u = ref.tower_forward(model.user_encoder, users, uf, training=False)
        p = ref.tower_forward(model.item_encoder, pos, pf, training=False)
        if mimic is not None:
            u = ref.gather_aug(mimic.user_augmented, users, u)[0]
            p = ref.gather_aug(mimic.item_augmented, pos, p)[0]
        pos_logits = (u * p).sum(dim=-1)
        nf = item_features.index_select(0, neg_flat) if has_i else None
        n = ref.tower_forward(model.item_encoder, neg_flat, nf, training=False)
        if mimic is not None:
            n = ref.gather_aug(mimic.item_augmented, neg_flat, n)[0]
        n = n.view(users.shape[0], -1, u.shape[-1])
        neg_logits = (u.unsqueeze(1) * n).sum(dim=-1)
        logits = torch.cat([pos_logits, neg_logits.reshape(-1)], dim=0)
        labels = torch.cat([torch.ones_like(pos_logits), torch.zeros_like(neg_logits.reshape(-1))], dim=0)
        loss = F.binary_cross_entropy_with_logits(logits, labels)
    return float(loss.item()), logits


def _engine(prob, model, *, max_batch=None, seed=7, positives=True):
    return ttamm.FusedEvalLoss(
        model, negatives_per_positive=prob.shape.N, positives=prob.positives if positives else None,
        user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
        max_batch=max_batch or prob.shape.B, seed=seed)


def _close(got: float, want: float, tol: float) -> bool:
    return abs(got - want) <= tol * abs(want)


CASES = {
    "tiny": Shape(),  # generic scorer at D = 8; dropout 0.15 in the config must not apply
    "c2dims": Shape(U=300, I=2000, F=605, H=192, D=96, hidden_dims=(192,), B=67, N=5),
    "n9": Shape(U=64, I=512, F=20, H=32, D=32, hidden_dims=(32,), B=33, N=9),
    "n1": Shape(U=64, I=512, F=20, H=32, D=32, hidden_dims=(32,), B=33, N=1),
    "odd": Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, gate_hidden=20, hidden_dims=(24, 16)),
    "nomimic": Shape(mimic=False),
    "sum": Shape(fusion="sum"),
    "concat": Shape(fusion="concat"),
    "concat-out28": Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, hidden_dims=(24,), fusion="concat",
                          feature_out=20, concat_out=28),
    "identity-enc": Shape(F=8, feature_type="identity"),
    "linear-enc": Shape(feature_type="linear"),
    "gelu": Shape(activation="gelu"),
    "padding": Shape(padding_idx=5),
    "max-norm": Shape(sparse=False, max_norm=0.05),
    "bf16": Shape(matmul_dtype="bf16"),
    "bf16-d128": Shape(U=300, I=2000, F=64, H=128, D=128, B=150, N=3, hidden_dims=(128,), matmul_dtype="bf16"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_logits_match_oracle_and_nothing_else_moves(case):
    from gpu_helpers import ttamm_model_from

    shape = CASES[case]
    prob = make_problem(shape, steps=1)
    users, pos, neg, _, _ = prob.batches[0]
    om = clone_model(prob.model)
    want_loss, want_logits = oracle_eval_batch(om, users, pos, neg, prob.user_features, prob.item_features)

    model = ttamm_model_from(prob).eval()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = _engine(prob, model)
    logits = torch.full((shape.B * (1 + shape.N),), float("nan"), device="cuda")
    eng.step(users.cuda(), pos.cuda(), neg.cuda(), logits_out=logits)
    last = eng.last_loss()
    got_loss = eng.finish()
    bf16 = shape.matmul_dtype == "bf16"
    err = rel_err(logits, want_logits)
    print(f"\n{case}: loss {got_loss:.8f} oracle {want_loss:.8f} rel {abs(got_loss - want_loss) / abs(want_loss):.2e}"
          f"  logits rel_err {err:.2e}")
    assert last == got_loss  # one batch: the pass's weighted mean is that batch's BCE
    assert _close(got_loss, want_loss, BF16_LOSS_TOL if bf16 else LOSS_TOL)
    assert err <= (BF16_LOGIT_TOL if bf16 else LOGIT_TOL)
    assert eng.loss_out.tolist() == [last, last, 0.0, 0.0, 0.0]

    after = model.state_dict()
    if shape.max_norm is None:
        for k, v in before.items():
            assert torch.equal(after[k], v), k
    else:
        # nn.Embedding(max_norm) renorms the looked-up rows in eval mode too: the same rows as the
        # oracle's own tables, to the same values (the row norm's summation order is the only freedom)
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


def test_reads_the_live_tables_after_deferred_training():
    """The engine holds pointers, not copies: built before training, it scores the trained (and
    flushed) tables afterwards."""
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    prob = make_problem(Shape(), steps=3)
    users, pos, neg, _, _ = prob.batches[0]
    model = ttamm_model_from(prob)
    ev = _engine(prob, model)
    ev.step(users.cuda(), pos.cuda(), neg.cuda())
    first = ev.finish()
    want_first, _ = oracle_eval_batch(clone_model(prob.model), users, pos, neg, prob.user_features, prob.item_features)
    assert _close(first, want_first, LOSS_TOL)

    opts = ttamm_optimizers(model)
    tr = ttamm.FusedTrainStep(model, opts, negatives_per_positive=prob.shape.N, positives=prob.positives,
                              user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                              loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, deferred_adamw=True)
    for (u, p, n, um, im) in prob.batches:
        tr.step(u.cuda(), p.cuda(), n.cuda().reshape(-1),
                keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})
    tr.finish()  # flushes the deferred tables

    ev.step(users.cuda(), pos.cuda(), neg.cuda())
    second = ev.finish()
    om, _, _ = run_oracle(prob)
    want, _ = oracle_eval_batch(om, users, pos, neg, prob.user_features, prob.item_features)
    print(f"\nbefore training {first:.8f}, after {second:.8f} (oracle {want:.8f})")
    assert _close(second, want, LOSS_TOL)
    assert second != first


def test_multi_batch_pass_through_compute_loss():
    from gpu_helpers import ttamm_model_from

    prob = make_problem(Shape(), steps=3)
    sizes = (32, 32, 13)  # the last batch short, as drop_last=False leaves it
    batches = [(u[:s], p[:s], n[:s]) for (u, p, n, _, _), s in zip(prob.batches, sizes)]
    om = clone_model(prob.model)
    per = [oracle_eval_batch(om, u, p, n, prob.user_features, prob.item_features)[0] for u, p, n in batches]
    want = sum(l * s for l, s in zip(per, sizes)) / sum(sizes)

    model = ttamm_model_from(prob)
    assert model.training
    dev = torch.device("cuda")
    kw = dict(criterion=nn.BCEWithLogitsLoss(), negatives_per_positive=prob.shape.N, num_items=prob.shape.I,
              user_positive_items=prob.positives, user_features=prob.user_features.cuda(),
              item_features=prob.item_features.cuda(), device=dev)
    seen = []

    def hook(step, users, pos):
        seen.append((step, users.numel()))
        return batches[step][2], None  # a second element (train_one_epoch's keep masks) is ignored

    got = ttamm.compute_loss(model, [(u, p) for u, p, _ in batches], batch_hook=hook, **kw)
    assert seen == [(0, 32), (1, 32), (2, 13)]
    assert _close(got, want, LOSS_TOL), (got, want)
    assert not model.training

    loader = ttamm.DeviceInteractionLoader(torch.cat([u for u, _, _ in batches]).cuda(),
                                           torch.cat([p for _, p, _ in batches]).cuda(), 32, shuffle=False)
    got_dev = ttamm.compute_loss(model, loader, batch_hook=lambda step, users, pos: batches[step][2], **kw)
    assert got_dev == got  # the same batches: the same bits

    assert ttamm.compute_loss(model, [], **kw) == 0.0

    # one engine, two loaders: the second pass starts from zero
    eng = _engine(prob, model)
    for k in (0, 1):
        u, p, n = batches[k]
        eng.step(u.cuda(), p.cuda(), n.cuda())
        assert _close(eng.finish(), per[k], LOSS_TOL), k
    assert eng.finish() == 0.0


def test_sampled_negatives_are_valid_reproducible_and_scored():
    from gpu_helpers import ttamm_model_from

    shape = Shape(I=256, N=5)
    prob = make_problem(shape, steps=1, positives_per_user=4)
    users, pos, _, _, _ = prob.batches[0]
    model = ttamm_model_from(prob)

    def run(seed):
        eng = _engine(prob, model, seed=seed)
        eng.step(users.cuda(), pos.cuda())
        neg = eng.neg_buffer[: shape.B * shape.N].cpu().view(shape.B, shape.N)
        return eng.finish(), neg

    loss, neg = run(11)
    assert int(neg.min()) >= 0 and int(neg.max()) < shape.I
    for b, u in enumerate(users.tolist()):
        assert not set(neg[b].tolist()) & prob.positives[u], (b, u)
    want, _ = oracle_eval_batch(clone_model(prob.model), users, pos, neg, prob.user_features, prob.item_features)
    assert _close(loss, want, LOSS_TOL), (loss, want)
    loss2, neg2 = run(11)
    assert loss2 == loss and torch.equal(neg2, neg)
    _, neg3 = run(12)
    assert not torch.equal(neg3, neg)


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
    first, _ = oracle_eval_batch(clone_model(prob.model), u0, p0, n0, prob.user_features, prob.item_features)
    total, count = eng.loss_accum.tolist()
    assert count == prob.shape.B  # exactly the first batch: the bad one and the one after it wrote nothing
    assert _close(total / count, first, LOSS_TOL)
    with pytest.raises(IndexError, match="index out of range in self"):
        eng.finish()
    assert eng.finish() == 0.0  # the raise left the engine clean

    u, p, n = u0.cuda(), p0.cuda(), n0.cuda()
    with pytest.raises(ValueError, match=r"negatives must be int64 \[batch, negatives_per_positive\]"):
        eng.step(u, p, n.reshape(-1)[:-1])
    with pytest.raises(ValueError, match=r"negatives must be int64 \[batch, negatives_per_positive\]"):
        eng.step(u, p, n.to(torch.int32))
    with pytest.raises(ValueError, match="batch larger than the step was sized for"):
        eng.step(torch.cat([u, u]), torch.cat([p, p]))
    with pytest.raises(ValueError, match="torch.long"):
        eng.step(u.to(torch.int32), p, n)
    with pytest.raises(RuntimeError, match="executes on an MI355X"):
        eng.step(u0, p0, n0)
    with pytest.raises(ValueError, match="positives are required to sample negatives"):
        _engine(prob, model, positives=False).step(u, p)
    assert eng.finish() == 0.0  # nothing was enqueued by the rejected calls


def test_c1_validation_loss_end_to_end():
    """The C1 fixture's validation pairs through compute_loss in batches of 512, on the untrained
    seeded weights, negatives from the reference sampler under a seeded generator."""
    from c1_helpers import N, TOWER_CFG, build_oracle_model, load_c1

    c1 = load_c1()
    om = build_oracle_model(c1)
    dev = torch.device("cuda")
    ue = ttamm.build_tower_encoder(dict(TOWER_CFG), num_embeddings=c1.num_users,
                                   feature_dim=c1.user_features.shape[1], device=dev)
    ie = ttamm.build_tower_encoder(dict(TOWER_CFG), num_embeddings=c1.num_items,
                                   feature_dim=c1.item_features.shape[1], device=dev)
    mm = ttamm.AdaptiveMimicMechanism(num_users=c1.num_users, num_items=c1.num_items,
                                      embedding_dim=ue.output_dim).to(dev)
    model = ttamm.TwoTowerModel(ue, ie, similarity=nn.CosineSimilarity(dim=-1), adaptive_mimic=mm)
    res = model.load_state_dict({k: v.to(dev) for k, v in om.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys

    pairs = torch.tensor(c1.val_pairs, dtype=torch.long)
    gen = torch.Generator().manual_seed(4321)
    batches = []
    for lo in range(0, pairs.shape[0], 512):
        u, p = pairs[lo:lo + 512, 0].contiguous(), pairs[lo:lo + 512, 1].contiguous()
        batches.append((u, p, ref.sample_negative_items(u, num_items=c1.num_items, positives=c1.positives,
                                                        num_negatives=N, generator=gen)))
    assert len(batches) > 1
    per = [oracle_eval_batch(om, u, p, n, c1.user_features, c1.item_features)[0] for u, p, n in batches]
    want = sum(l * u.numel() for l, (u, _, _) in zip(per, batches)) / pairs.shape[0]
    got = ttamm.compute_loss(
        model, [(u, p) for u, p, _ in batches], criterion=nn.BCEWithLogitsLoss(), negatives_per_positive=N,
        num_items=c1.num_items, user_positive_items=c1.positives, user_features=c1.user_features.to(dev),
        item_features=c1.item_features.to(dev), device=dev, batch_hook=lambda step, users, pos: (batches[step][2], None))
    print(f"\nC1 validation loss: ttamm {got:.8f} oracle {want:.8f} rel {abs(got - want) / abs(want):.2e}")
    assert _close(got, want, LOSS_TOL)
