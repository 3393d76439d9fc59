"""The drawn negative and dropout streams, decision by decision, against their CPU restatement
(oracle/philox.py; tests/test_philox_cpu.py checks that restatement on its own).

Every other parity test hands the kernels their random decisions; production draws them on the
device.  Here the production path is held to the restatement by exact equality, and through it to
the injected path the CPU oracle already checks at 1e-5:

  A. ttamm_sample_negatives (sampler.hip sample_negatives_kernel) through the ABI and the wrapper;
  B. the fused step's prologue (step_prologue_kernel) and the eval passes' sampler launch;
  C. the keep decisions of the three forward epilogues (gemm.hip epilogue8_hidden in gemm_x_kernel:
     the default split path, bf16 towers and pre-split feature planes; epilogue_hidden_pair in
     gemm_kernel: TTAMM_FP32_MFMA=exact) through ttamm_tower_train_forward / _backward;
  D. the whole step: drawn (production) run == injected run fed the restated decisions, bit for
     bit, and that injected run against the CPU oracle at the project's bounds (bf16 towers reach
     epilogue_hidden_pair in gemm_bf16_kernel there).

No expected value is recorded from a device run: every one is computed by oracle/philox.py."""

from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import ttamm
from helpers import LOSS_WEIGHTS, Shape, make_problem
from oracle import philox as px
from ttamm import _lib

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15  # a seed whose high word is not zero
COUNTER_HI = (1 << 32) + 3


# ---------------------------------------------------------------------------------------
# A. ttamm_sample_negatives
# ---------------------------------------------------------------------------------------
def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    val = np.array([x for v in lists for x in sorted(v)], dtype=np.int64)
    return off, val


def _csr_of(positives: dict, rows: int):
    return _csr([sorted(positives.get(u, ())) for u in range(rows)])


def _subsets(num_items, sizes, seed=11):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(num_items, size=s, replace=False).tolist()) for s in sizes]


def _device_sample(users, num_neg, num_items, off, val, user_rows, seed, counter, slot_base):
    """ttamm_sample_negatives -> (out int64 [batch, num_neg] on the host, status word)."""
    lib = _lib.load()
    users_d = torch.as_tensor(np.asarray(users, dtype=np.int64)).cuda()
    off_d = torch.as_tensor(off).cuda() if off is not None else None
    val_d = torch.as_tensor(val).cuda() if off is not None else None
    batch = users_d.numel()
    out = torch.full((batch, num_neg), -1, dtype=torch.long, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.ttamm_sample_negatives(
        users_d.data_ptr(), batch, num_neg, num_items, off_d.data_ptr() if off_d is not None else None,
        (val_d.data_ptr() or None) if val_d is not None else None, user_rows, seed, counter, slot_base,
        out.data_ptr(), status.data_ptr(), _lib.stream_handle(torch.device("cuda"))))
    torch.cuda.synchronize()
    return out.cpu(), int(status.item())


def _assert_negatives(got: torch.Tensor, want: np.ndarray, what: str) -> None:
    want_t = torch.from_numpy(want)
    if not torch.equal(got, want_t):
        bad = (got != want_t).nonzero()
        rows = [(int(b), int(j), int(got[b, j]), int(want[b, j])) for b, j in bad[:10].tolist()]
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.size} slots differ; (row, slot, device, restated): {rows}")


def test_sampler_abi_main_case():
    """Positive lists of 0, 1, 31, 32, 33 and 45 of 50 items (either side of the 32-entry register
    scan and the binary search), over seeds, counters and slot bases with and without high words."""
    num_items, num_neg, batch = 50, 5, 257
    lists = _subsets(num_items, [0, 1, 31, 32, 33, 45])
    off, val = _csr(lists)
    users = np.arange(batch, dtype=np.int64) * 5 % len(lists)  # (5 is coprime to 6: every row occurs)
    assert set(users.tolist()) == set(range(len(lists)))
    for seed in (0, SEED_HI):
        for counter in (0, 7, COUNTER_HI):
            for slot_base in (0, 12345, (1 << 32) + 11):
                want, exhausted = px.negatives(users, num_neg, num_items, off, val, len(lists), seed, counter, slot_base)
                got, status = _device_sample(users, num_neg, num_items, off, val, len(lists), seed, counter, slot_base)
                what = f"seed {seed:#x} counter {counter:#x} slot_base {slot_base:#x}"
                _assert_negatives(got, want, what)
                assert bool(status & _lib.STATUS_SAMPLER_EXHAUSTED) == bool(exhausted.any()), what


def test_sampler_abi_users_outside_csr():
    """Ids >= user_rows and ids < 0 take the no-positives draw; a NULL CSR gives everyone that draw."""
    num_items, num_neg = 50, 5
    lists = _subsets(num_items, [45, 33, 40])
    off, val = _csr(lists)
    users = np.array([0, 3, -1, 1, 1000, -5, 2, (1 << 40), -(1 << 40), 3, 2, -1] * 11, dtype=np.int64)
    free = px.negative_candidates(users.size * num_neg, num_items, SEED_HI, 7, 12345, 0).astype(np.int64).reshape(-1, num_neg)
    want, exhausted = px.negatives(users, num_neg, num_items, off, val, len(lists), SEED_HI, 7, 12345)
    outside = (users < 0) | (users >= len(lists))
    assert np.array_equal(want[outside], free[outside]) and not np.array_equal(want[~outside], free[~outside])
    got, status = _device_sample(users, num_neg, num_items, off, val, len(lists), SEED_HI, 7, 12345)
    _assert_negatives(got, want, "users outside the CSR")
    assert bool(status & _lib.STATUS_SAMPLER_EXHAUSTED) == bool(exhausted.any())
    want0, ex0 = px.negatives(users, num_neg, num_items, None, None, 0, SEED_HI, 7, 12345)
    assert np.array_equal(want0, free) and not ex0.any()
    got0, status0 = _device_sample(users, num_neg, num_items, None, None, 0, SEED_HI, 7, 12345)
    _assert_negatives(got0, want0, "NULL CSR")
    assert status0 == 0


@pytest.mark.parametrize("num_items", [2, (1 << 31) + 7, (1 << 40) + 1], ids=["2", "2^31+7", "2^40+1"])
def test_sampler_abi_large_item_counts(num_items):
    """The 64-bit multiply-high: candidates over item counts past 2^31 and 2^32."""
    users = np.zeros(257, dtype=np.int64)
    want, _ = px.negatives(users, 5, num_items, None, None, 0, SEED_HI, COUNTER_HI, (1 << 32) + 11)
    assert want.min() >= 0 and want.max() < num_items
    assert num_items == 2 or want.max() > num_items // 2 > (1 << 30)  # (the high words are in play)
    got, status = _device_sample(users, 5, num_items, None, None, 0, SEED_HI, COUNTER_HI, (1 << 32) + 11)
    _assert_negatives(got, want, f"num_items {num_items}")
    assert status == 0


def test_sampler_abi_retry_chain_to_its_last_draw():
    """One user with 40 of 50 items blocked, in 20 slots; the seed is chosen on the CPU so that a slot
    accepts its 11th (last) draw and none is exhausted: an off-by-one in the chain's length moves
    that slot or sets the status bit."""
    num_items, num_neg = 50, 5
    lists = _subsets(num_items, [40, 0, 3])
    off, val = _csr(lists)
    users = np.array([0, 1, 2, 1] * 4, dtype=np.int64)
    args = None
    for seed in range(SEED_HI, SEED_HI + 4000):  # a slot of user 0 ends on draw 11 with p = 0.02: ~16 seeds
        first = px.first_accepted_attempt(users, num_neg, num_items, off, val, len(lists), seed, 7, 0)
        if first.max() == px.MAX_DRAWS - 1:
            args = (users, num_neg, num_items, off, val, len(lists), seed, 7, 0)
            break
    assert args is not None, "no seed found"
    want, exhausted = px.negatives(*args)
    first = px.first_accepted_attempt(*args)
    assert (first == px.MAX_DRAWS - 1).any() and not exhausted.any()
    assert np.array_equal(want[first == 10],
                          px.negative_candidates(users.size * num_neg, num_items, seed, 7, 0, 10)
                          .astype(np.int64).reshape(-1, num_neg)[first == 10])
    got, status = _device_sample(*args)
    _assert_negatives(got, want, f"retries, seed {seed:#x}")
    assert status == 0


def test_sampler_abi_exhaustion_writes_the_last_candidate():
    """One user with 63 of 64 items blocked (0.84 of its slots exhaust), the others free: the
    device writes the 11th candidate into an exhausted slot and raises the status bit; with the
    blocked user left out of the batch the bit stays clear."""
    num_items, num_neg = 64, 5
    lists = [[i for i in range(64) if i != 17], [], [5, 6]]
    off, val = _csr(lists)
    users = np.array([0, 1, 2] * 30, dtype=np.int64)
    want, exhausted = px.negatives(users, num_neg, num_items, off, val, len(lists), 0, 0, 0)
    assert exhausted[users == 0].mean() > 0.6 and not exhausted[users != 0].any()
    last = px.negative_candidates(users.size * num_neg, num_items, 0, 0, 0, px.MAX_DRAWS - 1).astype(np.int64)
    assert np.array_equal(want[exhausted], last.reshape(-1, num_neg)[exhausted])
    got, status = _device_sample(users, num_neg, num_items, off, val, len(lists), 0, 0, 0)
    _assert_negatives(got, want, "exhaustion")
    assert status & _lib.STATUS_SAMPLER_EXHAUSTED
    users = np.array([1, 2] * 45, dtype=np.int64)
    want, exhausted = px.negatives(users, num_neg, num_items, off, val, len(lists), 0, 0, 0)
    assert not exhausted.any()
    got, status = _device_sample(users, num_neg, num_items, off, val, len(lists), 0, 0, 0)
    _assert_negatives(got, want, "no exhaustion")
    assert status == 0


@pytest.mark.parametrize("manual_seed", [0, 17])
def test_sampler_python_wrapper(manual_seed):
    """ttamm.sample_negative_items draws its seed from torch's generator (samplers.draw_seed) and
    samples with counter 0, slot base 0; negative user ids have no positives."""
    from ttamm.samplers import draw_seed

    num_items = 50
    # (at most 20 of 50 blocked: a slot exhausts with 0.4^11 = 4e-5, and the wrapper raises if one does)
    positives = {u: set(v) for u, v in enumerate(_subsets(num_items, [20, 0, 10, 1]))}
    users = np.array([0, -1, 1, 2, 3, -7, 0, 2] * 32 + [3], dtype=np.int64)
    torch.manual_seed(manual_seed)
    seed = draw_seed()
    off, val = _csr_of(positives, 4)
    want, exhausted = px.negatives(users, 5, num_items, off, val, 4, seed, 0, 0)
    assert not exhausted.any()
    torch.manual_seed(manual_seed)
    got = ttamm.sample_negative_items(torch.from_numpy(users), num_items=num_items, positives=positives,
                                      num_negatives=5, device=torch.device("cuda"))
    _assert_negatives(got.cpu(), want, f"wrapper under manual_seed({manual_seed})")


# ---------------------------------------------------------------------------------------
# B. the fused prologue and the eval passes
# ---------------------------------------------------------------------------------------
def test_train_step_prologue_negatives():
    """FusedTrainStep.step(users, pos) with nothing injected: 3400 x 5 = 17,000 slots, past the
    prologue's 64 x 256 threads, so its grid-stride loop runs a second pass; after step k the
    negatives are the restated ones of counter k."""
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    shape = Shape(dropout=0.0, B=3400, N=5)
    assert shape.B * shape.N > 64 * 256
    prob = make_problem(shape, steps=3)
    off, val = _csr_of(prob.positives, shape.U)
    model = ttamm_model_from(prob)
    opts = ttamm_optimizers(model, lr=1e-3)
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=shape.N, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=shape.B, seed=SEED_HI)
    for k, (users, pos, _, _, _) in enumerate(prob.batches):
        eng.step(users.cuda(), pos.cuda())
        torch.cuda.synchronize()
        got = eng.neg_buffer.cpu().reshape(shape.B, shape.N)
        want, exhausted = px.negatives(users.numpy(), shape.N, shape.I, off, val, shape.U, SEED_HI, k, 0)
        assert not exhausted.any()
        _assert_negatives(got, want, f"train step {k}")
    eng.finish()


@pytest.mark.parametrize("in_batch,num_neg", [(False, 5), (True, 2)], ids=["plain", "inbatch-n2"])
def test_eval_engine_negatives(in_batch, num_neg):
    """The validation engine behind ttamm.compute_loss (FusedEvalLoss): batch k of a pass draws the
    restated negatives of counter k, and a finished pass starts again at 0."""
    from gpu_helpers import ttamm_model_from

    shape = Shape(N=num_neg, B=45)
    prob = make_problem(shape, steps=2)
    off, val = _csr_of(prob.positives, shape.U)
    model = ttamm_model_from(prob).eval()
    eng = ttamm.training.FusedEvalLoss(model, negatives_per_positive=num_neg, positives=prob.positives,
                                       user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                                       max_batch=shape.B, seed=SEED_HI, in_batch_negatives=in_batch)
    for _ in range(2):  # two passes
        for k, (users, pos, _, _, _) in enumerate(prob.batches):
            eng.step(users.cuda(), pos.cuda())
            torch.cuda.synchronize()
            got = eng.neg_buffer.cpu().reshape(shape.B, num_neg)
            want, exhausted = px.negatives(users.numpy(), num_neg, shape.I, off, val, shape.U, SEED_HI, k, 0)
            assert not exhausted.any()
            _assert_negatives(got, want, f"eval batch {k}")
        eng.finish()


# ---------------------------------------------------------------------------------------
# C. the dropout stream in each forward kernel
# ---------------------------------------------------------------------------------------
DISPATCHES = ["split", "exact", "bf16", "planes"]


def _set_dispatch(monkeypatch, dispatch: str) -> None:
    if dispatch == "exact":
        monkeypatch.setenv("TTAMM_FP32_MFMA", "exact")
    else:
        monkeypatch.delenv("TTAMM_FP32_MFMA", raising=False)
    monkeypatch.delenv("TTAMM_GENERIC_GATE", raising=False)


def _planes_of(feats: torch.Tensor) -> torch.Tensor:
    """The rows' bf16 hi / mid / lo planes (ttamm_to_planes), as FusedTrainStep(feature_planes=True) keeps them."""
    rows, width = feats.shape
    ld = 48 * ((width + 15) // 16)
    out = torch.empty((rows, ld), dtype=torch.int16, device=feats.device)
    _lib.check(_lib.load().ttamm_to_planes(feats.data_ptr(), rows, width, feats.stride(0), out.data_ptr(), ld,
                                           _lib.stream_handle(feats.device)))
    return out


class _Run:
    """ttamm_tower_train_forward / _backward on a tower's rows with an explicit (seed, counter), or
    with injected keep masks (ttamm.autograd._TowerRun holds the descriptor and the workspace)."""

    def __init__(self, tower, idx, feats, dispatch, seed, counter, keep_masks=None, dropout=None):
        from ttamm.autograd import _TowerRun, _padded_rows

        self.feats = _padded_rows(feats)
        self.masks = [torch.from_numpy(m).cuda() for m in keep_masks] if keep_masks is not None else None
        self.run = _TowerRun(tower, idx, self.feats, seed, counter, self.masks)
        if dropout is not None:
            self.run.desc.dropout = dropout
        if dispatch == "planes":
            self.planes = _planes_of(self.feats)
            self.run.desc.features_planes = self.planes.data_ptr()
            self.run.desc.feat_planes_ld = self.planes.stride(0)

    def forward(self) -> torch.Tensor:
        out = self.run.forward()
        torch.cuda.synchronize()
        return out

    def backward(self, d_out: torch.Tensor):
        """(gradient arena, d_id_rows): the ABI's own outputs."""
        r = self.run
        n_arena = int(r.lib.ttamm_tower_grad_floats(ctypes.byref(r.desc)))
        arena = torch.zeros(max(1, n_arena), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros((r.n, r.tower.id_dim), dtype=torch.float32, device="cuda")
        _lib.check(r.lib.ttamm_tower_train_backward(
            ctypes.byref(r.desc), r.idx.data_ptr(), None, r.n, r.mask_arr, d_out.data_ptr(), arena.data_ptr(),
            d_rows.data_ptr(), None, r.ws.data_ptr(), r.ws.numel(), _lib.stream_handle(torch.device("cuda"))))
        torch.cuda.synchronize()
        return arena, d_rows


def _tower(shape: Shape, rows: int):
    enc = ttamm.build_tower_encoder(shape.tower_cfg(), num_embeddings=rows, feature_dim=shape.F, device="cuda")
    return enc.train()


def _positive_(t: torch.Tensor, lo: float, hi: float, gen: torch.Generator) -> None:
    with torch.no_grad():
        t.copy_((torch.rand(t.shape, generator=gen) * (hi - lo) + lo).to(t.device))


def _mask_tower(H: int, bf16: bool):
    """One hidden layer of width H, sum fusion, a zero ID table and an identity final Linear with zero
    bias; strictly positive layer-1 weights, bias and features: every pre-activation is > 0, so
    out[r, c] = relu(pre[r, c]) * keep[r, c] / (1 - p) and out != 0 IS the keep mask."""
    from ttamm.encoders import feature_layers

    shape = Shape(F=12, D=H, hidden_dims=(H,), fusion="sum", dropout=0.5, mimic=False,
                  matmul_dtype="bf16" if bf16 else "fp32")
    enc = _tower(shape, 8)
    gen = torch.Generator().manual_seed(H)
    l1, l2 = feature_layers(enc)[0]
    _positive_(l1.weight, 0.05, 1.0, gen)
    _positive_(l1.bias, 0.05, 1.0, gen)
    with torch.no_grad():
        enc.embedding.weight.zero_()
        l2.weight.copy_(torch.eye(H))
        l2.bias.zero_()
    return enc, shape, gen


# (no width was rejected by any of the four paths: all of 12, 20, 100, 264 run on each)
MASK_WIDTHS = {"split": [12, 20, 100, 264], "exact": [12, 20, 100, 264], "bf16": [12, 20, 100, 264],
               "planes": [12, 20, 100, 264]}


@pytest.mark.parametrize("dispatch", DISPATCHES)
def test_dropout_mask_recovered_from_forward(dispatch, monkeypatch):
    """The keep mask read back from the forward's output equals dropout_keep element by element:
    widths with H % 8 == 4 (the last column group is half a draw) and one with more than 32 column
    groups; 1, 63 and 257 rows (257: a second 128-row tile and a one-row tail, where the lane-pair
    epilogue's clamped partner draw must not leak); p at both ends of the threshold; a counter with
    a high word."""
    _set_dispatch(monkeypatch, dispatch)
    checked = 0
    for H in MASK_WIDTHS[dispatch]:
        enc, shape, gen = _mask_tower(H, bf16=dispatch == "bf16")
        for n in (1, 63, 257):
            feats = (torch.rand((n, shape.F), generator=gen) * 0.9 + 0.1).cuda()
            idx = (torch.arange(n) % 8).cuda()
            for p in (1e-5, 0.15, 0.5):
                for counter in (0, COUNTER_HI):
                    out = _Run(enc, idx, feats, dispatch, SEED_HI, counter, dropout=p).forward()
                    got = (out != 0).cpu().numpy()
                    keys = px.tower_row_keys(n)
                    want = px.dropout_keep(keys, H, p, SEED_HI, counter, px.TOWER_USER, 0).astype(bool)
                    if not np.array_equal(got, want):
                        bad = np.argwhere(got != want)
                        rows = [(int(r), int(c), int(keys[r]), bool(got[r, c])) for r, c in bad[:20]]
                        raise AssertionError(
                            f"{dispatch} H={H} n={n} p={p} counter={counter:#x}: {bad.shape[0]} of {want.size} keep "
                            f"decisions differ; (row, column, key, device keeps): {rows}")
                    # kept values carry the 1 / (1 - p) scale of a positive pre-activation
                    assert bool((out >= 0).all())
                    checked += want.size
    print(f"\n{dispatch}: {checked} keep decisions equal the restatement")


TOWER_CASES = {
    "relu-100-20": Shape(F=37, D=8, hidden_dims=(100, 20), dropout=0.3, activation="relu", mimic=False),
    "relu-12-24-8": Shape(F=37, D=8, hidden_dims=(12, 24, 8), dropout=0.3, activation="relu", mimic=False),
    "gelu-100-20": Shape(F=37, D=8, hidden_dims=(100, 20), dropout=0.3, activation="gelu", mimic=False),
    "gelu-12-24-8": Shape(F=37, D=8, hidden_dims=(12, 24, 8), dropout=0.3, activation="gelu", mimic=False),
}


@pytest.mark.parametrize("dispatch", DISPATCHES)
@pytest.mark.parametrize("case", list(TOWER_CASES))
def test_tower_drawn_equals_injected(case, dispatch, monkeypatch):
    """Forward + backward with the masks drawn (keep_masks NULL) and with the restated masks
    injected: out, the gradient arena and d_id_rows agree bit for bit.  gelu layers hand the drawn
    mask to the backward through mask_out; relu layers read it back as hv > 0, and run on all-positive
    pre-activations so a wrong decision cannot hide behind a dead unit.  Masks restated for the other
    tower id must change the result, or the comparison could not fail."""
    from ttamm.encoders import feature_layers

    _set_dispatch(monkeypatch, dispatch)
    shape = TOWER_CASES[case]
    if dispatch == "bf16":
        shape = Shape(**{**shape.__dict__, "matmul_dtype": "bf16"})
    n, rows = 257, 300
    gen = torch.Generator().manual_seed(len(case))
    torch.manual_seed(3)
    enc = _tower(shape, rows)
    feats = torch.randn((n, shape.F), generator=gen)
    if shape.activation == "relu":
        feats = feats.abs() + 0.1
        for layer in feature_layers(enc)[0][:-1]:
            _positive_(layer.weight, 0.02, 0.3, gen)
            _positive_(layer.bias, 0.05, 0.2, gen)
    feats = feats.cuda()
    idx = torch.randint(0, rows, (n,), generator=gen).cuda()
    d_out = torch.randn((n, shape.D), generator=gen).cuda()
    seed, counter = SEED_HI, COUNTER_HI

    def restated(tower_id):
        return [px.dropout_keep(px.tower_row_keys(n), h, shape.dropout, seed, counter, tower_id, l)
                for l, h in enumerate(shape.hidden_dims)]

    def run(masks):
        r = _Run(enc, idx, feats, dispatch, seed if masks is None else 0, counter if masks is None else 0, masks)
        out = r.forward()
        arena, d_rows = r.backward(d_out)
        return out, arena, d_rows

    drawn, injected, other = run(None), run(restated(px.TOWER_USER)), run(restated(px.TOWER_ITEM))
    for name, a, b in zip(("out", "gradient arena", "d_id_rows"), drawn, injected):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        assert diff == 0, f"{case} {dispatch} {name}: {diff} of {a.numel()} elements differ between drawn and injected"
    assert not torch.equal(drawn[0], other[0]) and not torch.equal(drawn[1], other[1])
    assert bool(drawn[1].abs().sum() > 0)


@pytest.mark.parametrize("side", ["user", "item"])
def test_module_path_draws_the_restated_mask(side):
    """ttamm.autograd.tower_train_forward under torch.manual_seed(17): its masks are the restated
    ones for seed = draw_seed() after the same manual_seed, counter 0 and tower 0 — for the item
    encoder as well (a lone tower has no tower id)."""
    from gpu_helpers import ttamm_model_from
    from ttamm.autograd import tower_params, tower_train_forward
    from ttamm.samplers import draw_seed

    shape = Shape(dropout=0.3)
    prob = make_problem(shape, steps=1)
    model = ttamm_model_from(prob).train()
    users, pos, _, _, _ = prob.batches[0]
    enc, idx, table = (model.user_encoder, users, prob.user_features) if side == "user" else \
        (model.item_encoder, pos, prob.item_features)
    idx = idx.cuda()
    feats = table.cuda()[idx]
    gy = torch.randn((idx.numel(), shape.D), generator=torch.Generator().manual_seed(2)).cuda()
    torch.manual_seed(17)
    seed = draw_seed()

    def run(keep_masks):
        for p in enc.parameters():
            p.grad = None
        torch.manual_seed(17)
        out = tower_train_forward(enc, idx, feats, keep_masks=keep_masks)
        out.backward(gy)
        torch.cuda.synchronize()
        return out.detach().clone(), [p.grad.clone() for p in tower_params(enc)[1:]]

    def restated(tower_id):
        return [torch.from_numpy(px.dropout_keep(px.tower_row_keys(idx.numel()), h, shape.dropout, seed, 0, tower_id, l)).cuda()
                for l, h in enumerate(shape.hidden_dims)]

    out_d, grads_d = run(None)
    out_i, grads_i = run(restated(px.TOWER_USER))
    assert torch.equal(out_d, out_i)
    assert len(grads_d) == len(grads_i) > 0
    for a, b in zip(grads_d, grads_i):
        assert torch.equal(a, b)
    out_o, _ = run(restated(px.TOWER_ITEM))
    assert not torch.equal(out_d, out_o)


# ---------------------------------------------------------------------------------------
# D. the whole step: production path == injected path, injected path vs the oracle
# ---------------------------------------------------------------------------------------
STEP_CASES = {
    "relu-100-20": (Shape(dropout=0.3, hidden_dims=(100, 20)), False),
    "gelu-16-12": (Shape(dropout=0.15, activation="gelu", hidden_dims=(16, 12)), False),
    "inbatch-n0": (Shape(N=0, dropout=0.3), True),
    # (beyond the three fp32 shapes: bf16 towers stream bf16 feature rows, the one route to
    # gemm_bf16_kernel's lane-pair epilogue; judged at the bf16 step's own oracle bounds)
    "bf16-100-20": (Shape(dropout=0.3, hidden_dims=(100, 20), matmul_dtype="bf16"), False),
}


def _restated_batches(prob, seed):
    """prob.batches with the negatives and keep masks the step draws for (seed, counter = step index)."""
    s = prob.shape
    off, val = _csr_of(prob.positives, s.U)
    out = []
    for k, (users, pos, _, _, _) in enumerate(prob.batches):
        neg, exhausted = px.negatives(users.numpy(), s.N, s.I, off, val, s.U, seed, k, 0) if s.N else \
            (np.zeros((s.B, 0), dtype=np.int64), np.zeros((s.B, 0), dtype=bool))
        assert not exhausted.any()
        um = [torch.from_numpy(px.dropout_keep(px.step_user_row_keys(s.B), h, s.dropout, seed, k, px.TOWER_USER, l))
              for l, h in enumerate(s.hidden_dims)]
        im = [torch.from_numpy(px.dropout_keep(px.step_item_row_keys(s.B, s.N), h, s.dropout, seed, k, px.TOWER_ITEM, l))
              for l, h in enumerate(s.hidden_dims)]
        out.append((users, pos, torch.from_numpy(neg), um, im))
    return out


def _run_drawn(prob, *, lr, betas, in_batch, seed):
    """The production path: FusedTrainStep(seed=), step(users, pos), nothing injected."""
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    model = ttamm_model_from(prob)
    opts = ttamm_optimizers(model, lr=lr, betas=betas)
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=prob.shape.N, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, in_batch_negatives=in_batch, seed=seed)
    losses = []
    for (users, pos, _, _, _) in prob.batches:
        eng.step(users.cuda(), pos.cuda())
        losses.append(eng.last_losses())
    eng.finish()
    return model, opts, losses


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_drawn_equals_injected_and_oracle(case, monkeypatch):
    """Three real steps (lr 1e-3): the drawn run and a fresh engine fed negatives(..) and
    dropout_keep(..) per step (counter = step index, tower 0 keys r for users, tower 1 keys r for
    positives and B + slot for negatives) give the same losses, parameters and optimizer state, bit for
    bit.  The injected run's first step at lr = 0, betas (0, 0.999) then meets
    test_gemm_paths_gpu._check_against_oracle's bounds against the CPU oracle's train_step on those
    restated inputs: the project's 1e-5 covers the drawn path, with no new tolerance."""
    from test_gemm_paths_gpu import _assert_same_run, _check_against_oracle, _run_engine, _set_mode

    _set_mode(monkeypatch, exact=False)
    shape, in_batch = STEP_CASES[case]
    seed = SEED_HI
    prob = make_problem(shape, steps=3)
    prob_i = dataclasses.replace(prob, batches=_restated_batches(prob, seed))
    drawn = _run_drawn(prob, lr=1e-3, betas=(0.9, 0.999), in_batch=in_batch, seed=seed)
    im, io, il, _ = _run_engine(prob_i, lr=1e-3, betas=(0.9, 0.999), in_batch=in_batch, seed=seed + 1)
    _assert_same_run(drawn, (im, io, il), f"{case}: drawn vs injected")
    # the restated decisions differ from make_problem's torch-drawn ones: the comparison is live
    if shape.N:
        assert not torch.equal(prob_i.batches[0][2], prob.batches[0][2])
    assert not torch.equal(prob_i.batches[0][4][0], prob.batches[0][4][0])
    first = dataclasses.replace(prob_i, batches=prob_i.batches[:1])
    tm, to, tl, _ = _run_engine(first, lr=0.0, betas=(0.0, 0.999), in_batch=in_batch, seed=seed + 1)
    worst = _check_against_oracle(first, tm, to, tl[0], in_batch=in_batch, bf16=shape.matmul_dtype == "bf16")
    print(f"\n{case}: injected restated inputs vs the oracle, worst rel_err {worst:.2e}")
