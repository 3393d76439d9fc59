"""The in-batch softmax objective (ttamm_inbatch_softmax, ttamm_inbatch_softmax_loss, the
in_batch_loss / in_batch_inv_temperature fields of ttamm_step_args and the Python keywords):
everything that is decided before any device work, in the manner of
tests/test_eval_loss_inbatch_cpu.py (the library loads without a GPU), and the float64 helper
against a dense F.cross_entropy."""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import ttamm
from helpers import Shape
from softmax_reference import inbatch_softmax_chunked
from ttamm import _lib
from ttamm.sharded import ShardedTrainStep

FAKE = 4096  # a never dereferenced pointer: every call here fails before anything is read


def _call_op(users=FAKE, batch=16, positives=FAKE, n_positives=16, dim=32, row_base=0, inv_t=1.0, du=FAKE, dp=FAKE,
             loss=FAKE, ws=FAKE, ws_bytes=1 << 24):
    return _lib.load().ttamm_inbatch_softmax(users, batch, dim, positives, n_positives, dim, dim, row_base, 1.0 / batch,
                                             inv_t, du, dim, dp, dim, loss, ws, ws_bytes, None)


def _call_loss(users=FAKE, batch=16, positives=FAKE, n_positives=16, dim=32, row_base=0, inv_t=1.0, loss=FAKE,
               ws=FAKE, ws_bytes=1 << 24):
    return _lib.load().ttamm_inbatch_softmax_loss(users, batch, dim, positives, n_positives, dim, dim, row_base, inv_t,
                                                  loss, ws, ws_bytes, None)


@pytest.mark.parametrize("call,nulls", [(_call_op, ("users", "positives", "du", "dp", "loss", "ws")),
                                        (_call_loss, ("users", "positives", "loss", "ws"))], ids=["op", "loss"])
def test_ops_reject_bad_arguments_before_any_device_work(call, nulls):
    for null in nulls:
        with pytest.raises(ValueError, match="null argument"):
            _lib.check(call(**{null: None}))
    with pytest.raises(ValueError, match="row_base"):
        _lib.check(call(batch=16, n_positives=20, row_base=8))
    with pytest.raises(ValueError, match="row_base"):
        _lib.check(call(row_base=-1))
    with pytest.raises(ValueError, match="multiple of 4"):
        _lib.check(call(dim=10))
    with pytest.raises(ValueError, match="multiple of 4, <= 128"):
        _lib.check(call(dim=132))
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(call(ws_bytes=0))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inverse temperature"):
            _lib.check(call(inv_t=bad))


def test_workspace_is_at_least_the_bce_ops_and_grows():
    lib = _lib.load()
    for B, Bc, D in ((16, 16, 32), (300, 300, 96), (8192, 8192, 96), (8192, 65536, 128)):
        sm = lib.ttamm_inbatch_softmax_workspace_size(B, Bc, D)
        fwd = lib.ttamm_inbatch_softmax_loss_workspace_size(B, Bc, D)
        assert sm >= lib.ttamm_inbatch_workspace_size(B, Bc, D) > 0
        assert 0 < fwd < sm
        assert lib.ttamm_inbatch_softmax_workspace_size(2 * B, Bc + B, D) > sm   # grows with B
        # and with Bc: the slabs' split plan caps its block count, so one doubling of the columns can
        # halve the splits and leave the bytes where they were (the BCE op's size does the same)
        assert lib.ttamm_inbatch_softmax_workspace_size(B, 2 * Bc, D) >= sm
        assert lib.ttamm_inbatch_softmax_workspace_size(B, 4 * Bc, D) > sm
        assert lib.ttamm_inbatch_softmax_loss_workspace_size(2 * B, Bc + B, D) > fwd
    # the forward-only pass holds pairs per row and split, never a [splits, B, D] slab
    assert lib.ttamm_inbatch_softmax_loss_workspace_size(8192, 8192, 96) < \
        lib.ttamm_inbatch_workspace_size(8192, 8192, 96) / 10
    assert lib.ttamm_inbatch_softmax_workspace_size(0, 16, 32) == 0
    assert lib.ttamm_inbatch_softmax_loss_workspace_size(16, 0, 32) == 0


def _fake_args(dim: int = 8, batch: int = 4, num_neg: int = 0) -> _lib.StepArgs:
    """Identity towers over fake table pointers, complete otherwise: the named field alone is at
    fault, and validation fails before anything is read."""
    args = _lib.StepArgs()
    for tower in (args.user, args.item):
        tower.id.weight = tower.id.exp_avg = tower.id.exp_avg_sq = FAKE
        tower.id.rows = 10
        tower.id.dim = dim
    args.b.batch = batch
    args.b.num_neg = num_neg
    args.in_batch = 1
    args.in_batch_loss = _lib.INBATCH_SOFTMAX
    args.in_batch_inv_temperature = 1.0
    args.hp.dense_step = args.hp.sparse_step = 1
    args.loss_out = args.status = args.workspace = FAKE
    args.b.users = args.b.pos_items = args.b.neg_items = FAKE
    args.workspace_bytes = 64
    return args


def _train(args):
    return _lib.load().ttamm_train_step(ctypes.byref(args), None)


def _eval(args):
    return _lib.load().ttamm_eval_loss_inbatch(ctypes.byref(args), None)


def test_step_args_default_is_todays_behaviour():
    args = _lib.StepArgs()
    assert args.in_batch_loss == _lib.INBATCH_BCE == 0 and args.in_batch_inv_temperature == 0.0
    assert _lib.INBATCH_SOFTMAX == 1


def test_well_formed_softmax_arguments_pass_validation():
    """Both entry points get as far as the workspace check."""
    for fn in (_train, _eval):
        with pytest.raises(ValueError, match="workspace too small"):
            _lib.check(fn(_fake_args()))


@pytest.mark.parametrize("what,match", [
    ("in_batch=0", "needs in_batch"),
    ("num_neg=2", "num_neg == 0"),
    ("phase", "phase == 0"),
    ("inv_t=0", "inverse temperature"),
    ("inv_t=-2", "inverse temperature"),
    ("inv_t=nan", "inverse temperature"),
    ("loss=7", "in_batch_loss must be"),
])
def test_train_step_rejects_softmax_misuse_by_name(what, match):
    args = _fake_args()
    if what == "in_batch=0":
        args.in_batch = 0
    elif what == "num_neg=2":
        args.b.num_neg = 2
    elif what == "phase":
        args.phase = _lib.PHASE_USER
    elif what.startswith("inv_t="):
        args.in_batch_inv_temperature = float(what[6:])
    elif what == "loss=7":
        args.in_batch_loss = 7
    with pytest.raises(ValueError, match=match):
        _lib.check(_train(args))


@pytest.mark.parametrize("what,match", [
    ("num_neg=2", "num_neg == 0"),
    ("phase", "phase"),
    ("inv_t=0", "inverse temperature"),
    ("inv_t=inf", "inverse temperature"),
    ("loss=7", "in_batch_loss must be"),
])
def test_eval_loss_inbatch_rejects_softmax_misuse_by_name(what, match):
    args = _fake_args()
    if what == "num_neg=2":
        args.b.num_neg = 2
    elif what == "phase":
        args.phase = _lib.PHASE_USER
    elif what.startswith("inv_t="):
        args.in_batch_inv_temperature = float(what[6:])
    elif what == "loss=7":
        args.in_batch_loss = 7
    with pytest.raises(ValueError, match=match):
        _lib.check(_eval(args))


def test_softmax_workspace_of_the_step_and_the_eval_pass_exceeds_bce():
    lib = _lib.load()
    args = _fake_args(dim=32, batch=300)
    sm_tr = lib.ttamm_train_step_workspace_size(ctypes.byref(args))
    sm_ev = lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args))
    args.in_batch_loss = _lib.INBATCH_BCE
    assert sm_tr > lib.ttamm_train_step_workspace_size(ctypes.byref(args)) > 0
    assert sm_ev > lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args)) > 0


def _model(shape: Shape):
    cfg = shape.tower_cfg()
    ue = ttamm.build_tower_encoder(cfg, num_embeddings=shape.U, feature_dim=shape.F)
    ie = ttamm.build_tower_encoder(cfg, num_embeddings=shape.I, feature_dim=shape.F)
    mm = ttamm.AdaptiveMimicMechanism(num_users=shape.U, num_items=shape.I, embedding_dim=shape.D)
    return ttamm.TwoTowerModel(ue, ie, similarity=ttamm.DotProductSimilarity(), adaptive_mimic=mm)


def _engines(model):
    kw = dict(positives=None, user_features=None, item_features=None, max_batch=8)
    return [lambda **k: ttamm.FusedTrainStep(model, [], **dict(kw, **k)),
            lambda **k: ttamm.FusedEvalLoss(model, **dict(kw, **k))]


def test_engine_keyword_errors_come_before_any_device_use():
    model = _model(Shape())  # on the CPU: anything that passes the argument checks hits a later check
    for make in _engines(model):
        with pytest.raises(ValueError, match="in_batch_loss must be 'bce' or 'softmax'"):
            make(negatives_per_positive=0, in_batch_negatives=True, in_batch_loss="hinge")
        with pytest.raises(ValueError, match="needs in_batch_negatives=True"):
            make(negatives_per_positive=2, in_batch_loss="softmax")
        with pytest.raises(ValueError, match="negatives_per_positive == 0"):
            make(negatives_per_positive=2, in_batch_negatives=True, in_batch_loss="softmax")
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature must be finite and greater than zero"):
                make(negatives_per_positive=0, in_batch_negatives=True, in_batch_loss="softmax", temperature=bad)
    # well-formed: construction goes on to the device check
    with pytest.raises(RuntimeError, match="executes on an MI355X"):
        ttamm.FusedEvalLoss(model, negatives_per_positive=0, in_batch_negatives=True, in_batch_loss="softmax",
                            temperature=0.25, positives=None, user_features=None, item_features=None, max_batch=8)


def test_drop_ins_check_the_keywords_before_touching_the_loader():
    model = _model(Shape())

    def loader():
        raise AssertionError("the loader was read")
        yield

    common = dict(criterion=torch.nn.BCEWithLogitsLoss(), num_items=256, user_features=None, item_features=None,
                  device=torch.device("cpu"))
    for fn, extra in ((ttamm.compute_loss, dict(user_positive_items=None)),
                      (ttamm.train_one_epoch, dict(user_positive_items={}, optimizers=[]))):
        kw = dict(common, **extra)
        with pytest.raises(ValueError, match="in_batch_loss must be"):
            fn(model, loader(), negatives_per_positive=0, in_batch_negatives=True, in_batch_loss="nce", **kw)
        with pytest.raises(ValueError, match="negatives_per_positive == 0"):
            fn(model, loader(), negatives_per_positive=3, in_batch_negatives=True, in_batch_loss="softmax", **kw)
        with pytest.raises(ValueError, match="needs in_batch_negatives=True"):
            fn(model, loader(), negatives_per_positive=3, in_batch_loss="softmax", **kw)
        with pytest.raises(ValueError, match="temperature must be"):
            fn(model, loader(), negatives_per_positive=0, in_batch_negatives=True, in_batch_loss="softmax",
               temperature=0.0, **kw)


def test_sharded_step_refuses_softmax_at_construction():
    model = _model(Shape())
    with pytest.raises(NotImplementedError, match="in_batch_loss='softmax' is not built for the row-sharded step"):
        ShardedTrainStep(model, [], world_size=2, rank=0, num_items=256, negatives_per_positive=0,
                         positives=None, user_features=None, item_features=None, max_batch=8,
                         in_batch_negatives=True, in_batch_loss="softmax")


def test_ops_check_the_temperature_and_the_device_first():
    u, p = torch.zeros((16, 32)), torch.zeros((16, 32))
    for fn in (ttamm.inbatch_softmax, ttamm.inbatch_softmax_loss):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature"):
                fn(u, p, temperature=bad)
        with pytest.raises(RuntimeError, match="executes on an MI355X"):
            fn(u, p)


def test_helper_is_the_dense_cross_entropy():
    g = torch.Generator().manual_seed(5)
    B, Bc, D, row_base, t = 50, 70, 12, 9, 0.3
    u = torch.randn((B, D), generator=g, dtype=torch.float64, requires_grad=True)
    p = torch.randn((Bc, D), generator=g, dtype=torch.float64, requires_grad=True)
    want = F.cross_entropy((u @ p.t()) / t, row_base + torch.arange(B), reduction="sum")
    (want / B).backward()
    for chunk in (1024, 16):  # one chunk, and four with a ragged last
        loss, du, dp = inbatch_softmax_chunked(u.detach(), p.detach(), row_base=row_base, temperature=t, chunk=chunk)
        assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
        assert (du - u.grad).abs().max().item() <= 1e-12 * u.grad.abs().max().item()
        assert (dp - p.grad).abs().max().item() <= 1e-12 * p.grad.abs().max().item()
