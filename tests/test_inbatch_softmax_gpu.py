"""The in-batch softmax cross-entropy as ops (ttamm.inbatch_softmax -> ttamm_inbatch_softmax: the
row log-sum-exp pass, ib_lse_merge_kernel, inbatch_x_kernel's softmax instantiation;
ttamm.inbatch_softmax_loss -> the LSE pass alone) against the chunked float64 evaluation of the
definition (tests/softmax_reference.inbatch_softmax_chunked).

Inputs as in tests/test_inbatch_loss_gpu.py: randn x scale, the own positive += boost x user, seed
B + Bc + D.  A case is (B, Bc, D, row_base, scale, boost, temperature).

Bounds: the project's 1e-5, relative on the loss sum and norm-wise (max|ours - fp64| / max|fp64|)
on dU and dP.  Two exceptions:
  * "minimum" (1 x 1): loss and gradients are exactly 0 in the definition, so they are compared
    absolutely, |loss| <= 1e-6 and |gradient| <= 1e-7;
  * "overflow-guard" (temperature 0.02, max |S / t| about 185: a sum of exp without the maximum
    subtracted is inf): the loss keeps 1e-5, but the logits' fp32 error is multiplied by
    1 / t = 50, and float32 torch on the CPU is itself several 1e-6 away from float64.  The test
    evaluates the helper in float32 on the CPU, E32 = max(dU, dP error) against float64, and asserts
    <= max(1e-5, 4 E32): the factor 4 covers the split-bf16 products, which do not keep all nine
    bf16 partial products.  E32 and the measured error are printed.  On the MI355X: E32 7.5e-6,
    bound 3.0e-5, measured dU 5.9e-6 / dP 6.2e-6 with the six partial products the softmax kernels
    keep; with the BCE kernels' five it was 5.8e-5 / 5.4e-5, over the bound, and the "temperature"
    case 1.004e-5 (profiles/inbatch_softmax_products.txt)."""

from __future__ import annotations

import functools

import pytest
import torch

import ttamm
from helpers import rel_err
from softmax_reference import inbatch_softmax_chunked

pytestmark = pytest.mark.gpu

TOL = 1e-5

CASES = {
    "minimum": (1, 1, 4, 0, 0.5, 0.5, 1.0),
    "one-tile": (64, 64, 64, 0, 0.3, 0.5, 1.0),
    "ragged-d12": (77, 77, 12, 0, 0.5, 0.5, 1.0),
    "second-128-row-block": (130, 130, 32, 0, 0.3, 0.5, 1.0),   # of the gradient kernel, two live rows
    "second-256-row-block": (258, 258, 32, 0, 0.3, 0.5, 1.0),   # of the LSE kernel
    "c2-dims": (300, 300, 96, 0, 0.3, 0.5, 1.0),                # several one-tile splits, ragged last
    "sharded-d128": (200, 900, 128, 450, 0.3, 0.5, 1.0),
    "label-in-last-partial-tile": (33, 700, 96, 667, 0.3, 0.5, 1.0),
    "multi-tile-splits": (40, 50000, 32, 49000, 0.3, 0.5, 1.0),  # the online rescale and the split merge
    "nine-row-blocks-two-tiles": (2100, 2100, 64, 0, 0.3, 0.5, 1.0),
    "temperature": (300, 300, 96, 0, 0.3, 0.5, 0.25),
    "overflow-guard": (200, 900, 64, 450, 0.3, 0.0, 0.02),
}


def _inputs(name: str):
    B, Bc, D, row_base, scale, boost, _ = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(B + Bc + D)
    users = torch.randn((B, D), device="cuda", generator=g) * scale
    pos = torch.randn((Bc, D), device="cuda", generator=g) * scale
    pos[row_base:row_base + B] += boost * users
    return users, pos


@functools.lru_cache(maxsize=None)
def _case(name: str):
    """(users, positives, float64 loss sum, dU, dP): computed once per case, shared by the tests,
    never written to."""
    row_base, t = CASES[name][3], CASES[name][6]
    users, pos = _inputs(name)
    want, du, dp = inbatch_softmax_chunked(users, pos, row_base=row_base, temperature=t)
    return users, pos, want, du, dp


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradients_match_fp64_definition(name):
    users, pos, want, du, dp = _case(name)
    row_base, t = CASES[name][3], CASES[name][6]
    loss, gu, gp = ttamm.inbatch_softmax(users, pos, row_base=row_base, temperature=t)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    got = float(loss)
    assert torch.isfinite(gu).all() and torch.isfinite(gp).all()
    if name == "minimum":
        print(f"\n{name}: loss {got:.3e} max|dU| {gu.abs().max().item():.3e} max|dP| {gp.abs().max().item():.3e}")
        assert want == 0.0 and not du.any() and not dp.any()
        assert abs(got) <= 1e-6
        assert gu.abs().max().item() <= 1e-7 and gp.abs().max().item() <= 1e-7
        return
    eu, ep = rel_err(gu, du), rel_err(gp, dp)
    bound = TOL
    if name == "overflow-guard":
        _, du32, dp32 = inbatch_softmax_chunked(users.cpu(), pos.cpu(), row_base=row_base, temperature=t,
                                                dtype=torch.float32)
        e32 = max(rel_err(du32, du), rel_err(dp32, dp))
        bound = max(TOL, 4.0 * e32)
        print(f"\n{name}: E32 {e32:.3e} bound {bound:.3e}")
        assert (users.double() @ pos.double().t()).abs().max().item() / t > 88.8  # exp overflows in fp32
    print(f"\n{name}: loss {got:.10e} fp64 {want:.10e} rel {abs(got - want) / abs(want):.2e} dU {eu:.2e} dP {ep:.2e}")
    assert abs(got - want) <= TOL * abs(want), (got, want)
    assert eu <= bound, f"dU rel err {eu:.3e} > {bound:.3e}"
    assert ep <= bound, f"dP rel err {ep:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_forward_only_is_the_training_ops_loss_and_both_are_bit_stable(name):
    users, pos = _case(name)[:2]
    row_base, t = CASES[name][3], CASES[name][6]
    a = ttamm.inbatch_softmax_loss(users, pos, row_base=row_base, temperature=t)
    b = ttamm.inbatch_softmax_loss(users, pos, row_base=row_base, temperature=t)
    l1, u1, p1 = ttamm.inbatch_softmax(users, pos, row_base=row_base, temperature=t)
    l2, u2, p2 = ttamm.inbatch_softmax(users, pos, row_base=row_base, temperature=t)
    assert a.dtype == torch.float64 and a.dim() == 0
    assert float(a) == float(b) == float(l1) == float(l2)  # one LSE pass, fixed-order sums
    assert torch.equal(u1, u2) and torch.equal(p1, p2)


def test_inv_count_scales_the_gradients_only():
    users, pos, want, du, dp = _case("c2-dims")
    loss, gu, gp = ttamm.inbatch_softmax(users, pos, inv_count=1.0)
    assert float(loss) == float(ttamm.inbatch_softmax_loss(users, pos))
    B = users.shape[0]
    assert rel_err(gu, du * B) <= TOL and rel_err(gp, dp * B) <= TOL


def test_every_row_of_ds_sums_to_zero():
    """All positives equal to one vector v: dU_b = (sum_j dS_bj) v = 0, and the rows of dP add up to
    sum_b (sum_j dS_bj) u_b = 0, whatever the logits."""
    g = torch.Generator(device="cuda").manual_seed(7)
    B, Bc, D = 130, 200, 32
    users = torch.randn((B, D), device="cuda", generator=g) * 0.3
    v = torch.randn((1, D), device="cuda", generator=g) * 0.3
    pos = v.expand(Bc, D).contiguous()
    _, gu, gp = ttamm.inbatch_softmax(users, pos, row_base=40)
    print(f"\nmax|dU| {gu.abs().max().item():.3e} max|sum_rows dP| {gp.double().sum(dim=0).abs().max().item():.3e}")
    assert gu.abs().max().item() <= 1e-7
    assert gp.double().sum(dim=0).abs().max().item() <= 1e-7


def test_strided_rows_are_read_through_their_leading_dimension():
    users, pos = _case("c2-dims")[:2]
    wide_u = torch.full((users.shape[0], 128), 7.0, device="cuda")
    wide_p = torch.full((pos.shape[0], 104), -3.0, device="cuda")
    wide_u[:, :96] = users
    wide_p[:, :96] = pos
    lib = ttamm._lib.load()
    B, Bc, D = users.shape[0], pos.shape[0], 96
    stream = ttamm._lib.stream_handle(users.device)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.ttamm_inbatch_softmax_loss_workspace_size(B, Bc, D)), dtype=torch.uint8, device="cuda")
    ttamm._lib.check(lib.ttamm_inbatch_softmax_loss(wide_u.data_ptr(), B, 128, wide_p.data_ptr(), Bc, 104, D, 0, 1.0,
                                                    loss.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    want, wu, wp = ttamm.inbatch_softmax(users, pos)
    assert float(loss) == float(want)
    # the training op: strided inputs and strided outputs, nothing written past D
    du = torch.full((B, 100), 5.0, device="cuda")
    dp = torch.full((Bc, 112), 6.0, device="cuda")
    ws = torch.empty(int(lib.ttamm_inbatch_softmax_workspace_size(B, Bc, D)), dtype=torch.uint8, device="cuda")
    ttamm._lib.check(lib.ttamm_inbatch_softmax(wide_u.data_ptr(), B, 128, wide_p.data_ptr(), Bc, 104, D, 0, 1.0 / B, 1.0,
                                               du.data_ptr(), 100, dp.data_ptr(), 112, loss.data_ptr(), ws.data_ptr(),
                                               ws.numel(), stream))
    assert float(loss) == float(want)
    assert torch.equal(du[:, :96], wu) and torch.equal(dp[:, :96], wp)
    assert bool((du[:, 96:] == 5.0).all()) and bool((dp[:, 96:] == 6.0).all())


def test_bad_shapes_dtypes_and_temperatures_raise():
    u = torch.zeros((16, 32), device="cuda")
    for fn in (ttamm.inbatch_softmax, ttamm.inbatch_softmax_loss):
        with pytest.raises(ValueError, match="one D"):
            fn(u, torch.zeros((16, 24), device="cuda"))
        with pytest.raises(ValueError, match="row_base"):
            fn(u, torch.zeros((20, 32), device="cuda"), row_base=8)
        with pytest.raises(ValueError, match="row_base"):
            fn(u, torch.zeros((20, 32), device="cuda"), row_base=-1)
        with pytest.raises(ValueError, match="float32"):
            fn(u.double(), torch.zeros((16, 32), device="cuda", dtype=torch.float64))
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(torch.zeros((16, 10), device="cuda"), torch.zeros((16, 10), device="cuda"))
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(torch.zeros((16, 132), device="cuda"), torch.zeros((16, 132), device="cuda"))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature"):
                fn(u, torch.zeros((16, 32), device="cuda"), temperature=bad)
        with pytest.raises(RuntimeError, match="executes on an MI355X"):
            fn(u.cpu(), torch.zeros((16, 32)))


def test_bce_ops_keep_their_bits_around_a_softmax_call():
    """No workspace state is shared: the BCE ops return the same bits before and after a softmax
    call on the same stream."""
    users, pos = _case("c2-dims")[:2]
    l0, u0, p0 = ttamm.inbatch_bce(users, pos)
    f0 = ttamm.inbatch_bce_loss(users, pos)
    ttamm.inbatch_softmax(users, pos, temperature=0.25)
    ttamm.inbatch_softmax_loss(users, pos, temperature=0.25)
    l1, u1, p1 = ttamm.inbatch_bce(users, pos)
    f1 = ttamm.inbatch_bce_loss(users, pos)
    assert float(l0) == float(l1) and float(f0) == float(f1)
    assert torch.equal(u0, u1) and torch.equal(p0, p1)
