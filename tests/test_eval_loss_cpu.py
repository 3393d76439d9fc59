"""ttamm_eval_loss / ttamm.compute_loss: everything that is decided before any device work (the
library loads without a GPU, as tests/test_abi_cpu.py shows)."""

from __future__ import annotations

import ctypes

import pytest
import torch

import ttamm
from helpers import Shape
from ttamm import _lib


def _fake_args() -> _lib.StepArgs:
    """Identity towers over fake, never dereferenced table pointers: validation fails (or the size
    query returns) before anything is read."""
    args = _lib.StepArgs()
    fake = 4096
    for tower in (args.user, args.item):
        tower.id.weight = fake
        tower.id.rows = 10
        tower.id.dim = 8
    args.b.batch = 4
    args.b.num_neg = 2
    return args


def test_null_and_empty_descriptors_are_rejected():
    lib = _lib.load()
    with pytest.raises(ValueError, match="null step args"):
        _lib.check(lib.ttamm_eval_loss(None, None, None))
    assert lib.ttamm_eval_loss_workspace_size(None) == 0
    with pytest.raises(ValueError, match="embedding table"):
        _lib.check(lib.ttamm_eval_loss(ctypes.byref(_lib.StepArgs()), None, None))


@pytest.mark.parametrize("field,value,match", [
    ("in_batch", 1, "in_batch"),
    ("phase", _lib.PHASE_USER, "phase"),
    ("num_neg", 0, "num_neg"),
    ("num_neg", 65, "num_neg"),
])
def test_out_of_scope_fields_are_rejected_by_name(field, value, match):
    lib = _lib.load()
    args = _fake_args()
    if field == "num_neg":
        args.b.num_neg = value
    else:
        setattr(args, field, value)
    with pytest.raises(ValueError, match=match):
        _lib.check(lib.ttamm_eval_loss(ctypes.byref(args), None, None))


def test_missing_outputs_and_workspace_are_rejected():
    lib = _lib.load()
    args = _fake_args()
    with pytest.raises(ValueError, match="loss_out, status and workspace"):
        _lib.check(lib.ttamm_eval_loss(ctypes.byref(args), None, None))
    args.loss_out = args.status = args.workspace = 4096
    args.b.users = args.b.pos_items = args.b.neg_items = 4096
    args.workspace_bytes = 64
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(lib.ttamm_eval_loss(ctypes.byref(args), None, None))


def test_workspace_is_positive_and_smaller_than_the_training_step():
    """No backward buffers, gradient slabs or coalesce scratch: the forward-only workspace is a
    strict part of what the training step needs for the same descriptor."""
    lib = _lib.load()
    args = _fake_args()
    for tower in (args.user, args.item):  # the training step's validation wants optimizer state
        tower.id.exp_avg = tower.id.exp_avg_sq = 4096
    ev = lib.ttamm_eval_loss_workspace_size(ctypes.byref(args))
    tr = lib.ttamm_train_step_workspace_size(ctypes.byref(args))
    assert 0 < ev < tr
    # ... and grows with the batch
    args.b.batch = 8
    assert lib.ttamm_eval_loss_workspace_size(ctypes.byref(args)) > ev


def _model(shape: Shape):
    cfg = shape.tower_cfg()
    ue = ttamm.build_tower_encoder(cfg, num_embeddings=shape.U, feature_dim=shape.F)
    ie = ttamm.build_tower_encoder(cfg, num_embeddings=shape.I, feature_dim=shape.F)
    mm = ttamm.AdaptiveMimicMechanism(num_users=shape.U, num_items=shape.I, embedding_dim=shape.D)
    return ttamm.TwoTowerModel(ue, ie, similarity=ttamm.DotProductSimilarity(), adaptive_mimic=mm)


def test_compute_loss_rejects_unsupported_options_before_any_device_use():
    model = _model(Shape())
    kw = dict(negatives_per_positive=2, user_positive_items={}, user_features=None, item_features=None,
              device=torch.device("cpu"))
    batch = [(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))]
    with pytest.raises(NotImplementedError, match="BCEWithLogitsLoss"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(reduction="sum"), num_items=256, **kw)
    with pytest.raises(NotImplementedError, match="BCEWithLogitsLoss"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)),
                           num_items=256, **kw)
    with pytest.raises(ValueError, match="num_items does not match"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(), num_items=255, **kw)
    assert not model.training  # eval mode, as the reference leaves it (training.py:848)
    assert ttamm.compute_loss(model, [], criterion=torch.nn.BCEWithLogitsLoss(), num_items=256, **kw) == 0.0
