"""ttamm_eval_loss_inbatch / ttamm_inbatch_bce_loss / compute_loss(in_batch_negatives=True):
everything that is decided before any device work (the library loads without a GPU, as
tests/test_abi_cpu.py shows)."""

from __future__ import annotations

import ctypes

import pytest
import torch

import ttamm
from helpers import Shape
from ttamm import _lib


def _fake_args(dim: int = 8, batch: int = 4, num_neg: int = 2) -> _lib.StepArgs:
    """Identity towers over fake, never dereferenced table pointers: validation fails (or the size
    query returns) before anything is read."""
    args = _lib.StepArgs()
    fake = 4096
    for tower in (args.user, args.item):
        tower.id.weight = fake
        tower.id.rows = 10
        tower.id.dim = dim
    args.b.batch = batch
    args.b.num_neg = num_neg
    return args


def _with_outputs(args: _lib.StepArgs) -> _lib.StepArgs:
    args.loss_out = args.status = args.workspace = 4096
    args.b.users = args.b.pos_items = args.b.neg_items = 4096
    args.workspace_bytes = 64
    return args


def test_null_descriptor_is_rejected():
    lib = _lib.load()
    with pytest.raises(ValueError, match="null step args"):
        _lib.check(lib.ttamm_eval_loss_inbatch(None, None))
    assert lib.ttamm_eval_loss_inbatch_workspace_size(None) == 0


@pytest.mark.parametrize("what,match", [
    ("phase", "phase"),
    ("num_neg=-1", "num_neg"),
    ("num_neg=65", "num_neg"),
    ("dim=10", r"embedding_dim % 4 == 0"),  # every tower's own limit, met first
    ("dim=132", "embedding dim must be a multiple of 4, <= 128"),
    ("empty", "empty batch"),
])
def test_out_of_scope_fields_are_rejected_by_name(what, match):
    lib = _lib.load()
    args = _fake_args(dim=int(what[4:]) if what.startswith("dim=") else 8)
    if what == "phase":
        args.phase = _lib.PHASE_USER
    elif what.startswith("num_neg="):
        args.b.num_neg = int(what[8:])
    elif what == "empty":
        args.b.batch = 0
    _with_outputs(args)  # complete otherwise: the named field alone is at fault
    with pytest.raises(ValueError, match=match):
        _lib.check(lib.ttamm_eval_loss_inbatch(ctypes.byref(args), None))


def test_in_batch_field_is_not_consulted_and_zero_negatives_are_legal():
    """num_neg = 0 (and either value of in_batch) passes validation: the call gets as far as the
    workspace check."""
    lib = _lib.load()
    for in_batch in (0, 1):
        args = _with_outputs(_fake_args(num_neg=0))
        args.in_batch = in_batch
        with pytest.raises(ValueError, match="workspace too small"):
            _lib.check(lib.ttamm_eval_loss_inbatch(ctypes.byref(args), None))


def test_missing_outputs_and_workspace_are_rejected():
    lib = _lib.load()
    args = _fake_args()
    with pytest.raises(ValueError, match="loss_out, status and workspace"):
        _lib.check(lib.ttamm_eval_loss_inbatch(ctypes.byref(args), None))
    _with_outputs(args)
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(lib.ttamm_eval_loss_inbatch(ctypes.byref(args), None))


def test_workspace_is_positive_smaller_than_the_training_step_and_grows():
    lib = _lib.load()
    args = _fake_args()
    for tower in (args.user, args.item):  # the training step's validation wants optimizer state
        tower.id.exp_avg = tower.id.exp_avg_sq = 4096
    ev = lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args))
    args.in_batch = 1
    tr = lib.ttamm_train_step_workspace_size(ctypes.byref(args))
    assert 0 < ev < tr
    args.b.batch = 8
    assert lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args)) > ev


@pytest.mark.parametrize("B", [4, 300, 8192])
def test_workspace_adds_block_partials_only(B):
    """The in-batch pass's workspace is the plain pass's plus one float per block of
    inbatch_loss_kernel: fewer than B / 32 + 1024 floats, so no [splits, B, D] slab crept in."""
    lib = _lib.load()
    args = _fake_args(dim=96, batch=B, num_neg=5)
    plain = lib.ttamm_eval_loss_workspace_size(ctypes.byref(args))
    ib = lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args))
    assert plain > 0
    assert 0 < ib - plain < 4 * (B // 32 + 1024), (ib, plain)


def test_inbatch_bce_loss_rejects_bad_arguments():
    lib = _lib.load()
    fake = 4096

    def call(users=fake, batch=16, positives=fake, n_positives=16, dim=32, row_base=0, loss=fake, ws=fake,
             ws_bytes=1 << 20):
        return lib.ttamm_inbatch_bce_loss(users, batch, dim, positives, n_positives, dim, dim, row_base, loss, ws,
                                          ws_bytes, None)

    for null in ("users", "positives", "loss", "ws"):
        with pytest.raises(ValueError, match="null argument"):
            _lib.check(call(**{null: None}))
    with pytest.raises(ValueError, match="row_base"):
        _lib.check(call(batch=16, n_positives=20, row_base=8))
    with pytest.raises(ValueError, match="row_base"):
        _lib.check(call(row_base=-1))
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(call(ws_bytes=0))
    with pytest.raises(ValueError, match="multiple of 4"):
        _lib.check(call(dim=10))


def test_op_workspace_holds_block_partials_only():
    lib = _lib.load()
    loss_only = lib.ttamm_inbatch_loss_workspace_size(8192, 8192, 96)
    full = lib.ttamm_inbatch_workspace_size(8192, 8192, 96)
    assert 0 < loss_only < full / 100
    assert lib.ttamm_inbatch_loss_workspace_size(0, 16, 32) == 0


def _model(shape: Shape):
    cfg = shape.tower_cfg()
    ue = ttamm.build_tower_encoder(cfg, num_embeddings=shape.U, feature_dim=shape.F)
    ie = ttamm.build_tower_encoder(cfg, num_embeddings=shape.I, feature_dim=shape.F)
    mm = ttamm.AdaptiveMimicMechanism(num_users=shape.U, num_items=shape.I, embedding_dim=shape.D)
    return ttamm.TwoTowerModel(ue, ie, similarity=ttamm.DotProductSimilarity(), adaptive_mimic=mm)


def test_engine_argument_errors_come_before_any_device_use():
    model = _model(Shape())  # on the CPU: anything that passes the argument checks hits require_rocm
    kw = dict(positives=None, user_features=None, item_features=None, max_batch=8)
    with pytest.raises(ValueError, match="num_negatives must be greater than zero"):
        ttamm.FusedEvalLoss(model, negatives_per_positive=-1, in_batch_negatives=True, **kw)
    with pytest.raises(ValueError, match="num_negatives must be greater than zero"):
        ttamm.FusedEvalLoss(model, negatives_per_positive=0, **kw)
    with pytest.raises(ValueError, match="num_negatives must be greater than zero"):
        ttamm.FusedEvalLoss(model, negatives_per_positive=0, in_batch_negatives=False, **kw)
    # N = 0 is legal in in-batch mode: construction goes on to the device check
    with pytest.raises(RuntimeError, match="executes on an MI355X"):
        ttamm.FusedEvalLoss(model, negatives_per_positive=0, in_batch_negatives=True, **kw)
    # an embedding dim the kernel cannot take: ValueError at construction, before any launch
    bad = _model(Shape(U=20, I=30, F=6, H=10, D=10, hidden_dims=(10,), gate_hidden=10))
    with pytest.raises(ValueError, match="embedding dim must be a multiple of 4, <= 128"):
        ttamm.FusedEvalLoss(bad, negatives_per_positive=2, in_batch_negatives=True, **kw)


def test_compute_loss_forwards_the_flag_and_keeps_its_checks():
    model = _model(Shape())
    kw = dict(user_features=None, item_features=None, device=torch.device("cpu"), in_batch_negatives=True)
    batch = [(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))]
    with pytest.raises(NotImplementedError, match="BCEWithLogitsLoss"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(reduction="sum"), num_items=256,
                           negatives_per_positive=0, user_positive_items=None, **kw)
    with pytest.raises(ValueError, match="num_items does not match"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(), num_items=255,
                           negatives_per_positive=0, user_positive_items=None, **kw)
    with pytest.raises(ValueError, match="num_negatives must be greater than zero"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(), num_items=256,
                           negatives_per_positive=-2, user_positive_items={}, **kw)
    # N = 0 with no positives map at all reaches the engine's device check
    with pytest.raises(RuntimeError, match="executes on an MI355X"):
        ttamm.compute_loss(model, batch, criterion=torch.nn.BCEWithLogitsLoss(), num_items=256,
                           negatives_per_positive=0, user_positive_items=None, **kw)
    assert not model.training
    assert ttamm.compute_loss(model, [], criterion=torch.nn.BCEWithLogitsLoss(), num_items=256,
                              negatives_per_positive=0, user_positive_items=None, **kw) == 0.0
