"""The forward-only in-batch BCE sum as one op (ttamm.inbatch_bce_loss -> ttamm_inbatch_bce_loss ->
inbatch_loss_kernel) against the chunked float64 evaluation of the oracle's in-batch definition
(oracle/cpu_reference.inbatch_bce_chunked), and against the training kernel (ttamm.inbatch_bce).

Tolerance: the project's 1e-5 relative on the sum (tests/test_inbatch_op_gpu.py); both kernels are
within 1e-5 of the float64 value, hence 2e-5 of each other.  Inputs as in that file: randn x scale,
the own positive += 0.5 x user.

The kernel's plan (inbatch_loss_plan): row blocks of 256 users x column splits of whole 64-column
tiles, about 256 blocks.  Per case, with rblk = ceil(B / 256):
    want = min(ceil(Bc / 64), ceil(256 / rblk)); cols = 64 ceil(ceil(Bc / want) / 64);
    splits = ceil(Bc / cols)
which the test restates (``_plan``) and prints.  The issue's seven shapes all give one-tile splits;
a further case puts two live rows into a second 256-row block, and two more reach the tile loop
(double buffering, the tile after next in flight): four tiles per split with a ragged 80-column
last split, and nine row blocks x 17 splits of two tiles."""

from __future__ import annotations

import functools

import pytest
import torch

import ttamm
from oracle import cpu_reference as ref

pytestmark = pytest.mark.gpu

TOL = 1e-5

CASES = {
    "minimum": (1, 1, 4, 0),
    "one-tile": (64, 64, 64, 0),
    "ragged-d12": (77, 77, 12, 0),
    "fifth-wave-two-live-rows": (130, 130, 32, 0),  # two row blocks of the 128-row training kernel
    "c2-dims": (300, 300, 96, 0),
    "sharded-d128": (200, 900, 128, 450),
    "label-in-last-partial-tile": (33, 700, 96, 667),
    "two-row-blocks": (258, 258, 32, 0),  # the second 256-row block with two live rows
    "four-tiles-ragged-split": (40, 50000, 32, 49000),
    "nine-row-blocks-two-tiles": (2100, 2100, 64, 0),
}


def _plan(B: int, Bc: int) -> tuple[int, int, int]:
    """(row blocks, column splits, columns per split) of inbatch_loss_plan."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    rblk = cdiv(B, 256)
    want = min(cdiv(Bc, 64), cdiv(256, rblk))
    cols = cdiv(cdiv(Bc, want), 64) * 64
    return rblk, cdiv(Bc, cols), cols


@functools.lru_cache(maxsize=None)
def _case(name: str):
    """(users, positives, float64 BCE sum): computed once per case, shared by the tests, never
    written to."""
    B, Bc, D, row_base = CASES[name]
    scale = 0.5 if D <= 16 else 0.3
    g = torch.Generator(device="cuda").manual_seed(B + Bc + D)
    users = torch.randn((B, D), device="cuda", generator=g) * scale
    pos = torch.randn((Bc, D), device="cuda", generator=g) * scale
    pos[row_base:row_base + B] += 0.5 * users
    want, _, _ = ref.inbatch_bce_chunked(users, pos, row_base=row_base, inv_count=1.0 / (B * Bc))
    return users, pos, float(want)


def test_the_cases_reach_every_path_of_the_plan():
    plans = {name: _plan(B, Bc) for name, (B, Bc, _, _) in CASES.items()}
    print("\n" + "\n".join(f"{n}: rblk {p[0]} splits {p[1]} cols {p[2]}" for n, p in plans.items()))
    lib = ttamm._lib.load()
    for name, (B, Bc, D, _) in CASES.items():
        rblk, splits, _ = plans[name]
        assert lib.ttamm_inbatch_loss_workspace_size(B, Bc, D) == 4 * rblk * splits, name
    # more than one column split with a ragged last split, one-tile and multi-tile
    B, Bc = CASES["c2-dims"][:2]
    assert plans["c2-dims"][1] > 1 and plans["c2-dims"][2] == 64 and Bc % 64 != 0
    assert plans["four-tiles-ragged-split"] == (1, 196, 256) and 50000 - 195 * 256 == 80
    assert plans["nine-row-blocks-two-tiles"] == (9, 17, 128) and 2100 - 16 * 128 == 52
    assert plans["two-row-blocks"][0] == 2 and plans["fifth-wave-two-live-rows"][0] == 1


@pytest.mark.parametrize("name", list(CASES))
def test_loss_sum_matches_fp64_definition_bit_stably(name):
    users, pos, want = _case(name)
    B, Bc, D, row_base = CASES[name]
    got = ttamm.inbatch_bce_loss(users, pos, row_base=row_base)
    again = ttamm.inbatch_bce_loss(users, pos, row_base=row_base)
    assert got.dtype == torch.float64 and got.dim() == 0
    g, a = float(got), float(again)
    print(f"\n{name}: plan {_plan(B, Bc)} got {g:.10e} fp64 {want:.10e} rel {abs(g - want) / abs(want):.2e}")
    assert abs(g - want) <= TOL * abs(want), (g, want)
    assert g == a  # fixed-order sums: the same inputs give the same bits


@pytest.mark.parametrize("name", list(CASES))
def test_loss_sum_agrees_with_the_training_kernel(name):
    users, pos, want = _case(name)
    B, Bc, D, row_base = CASES[name]
    got = float(ttamm.inbatch_bce_loss(users, pos, row_base=row_base))
    train = float(ttamm.inbatch_bce(users, pos, row_base=row_base)[0])
    print(f"\n{name}: forward-only {got:.10e} training kernel {train:.10e} rel {abs(got - train) / abs(want):.2e}")
    assert abs(got - train) <= 2e-5 * abs(want), (got, train, want)


def test_strided_rows_are_read_through_their_leading_dimension():
    users, pos, want = _case("c2-dims")
    wide_u = torch.full((users.shape[0], 128), 7.0, device="cuda")
    wide_p = torch.full((pos.shape[0], 104), -3.0, device="cuda")
    wide_u[:, :96] = users
    wide_p[:, :96] = pos
    lib = ttamm._lib.load()
    B, Bc, D = users.shape[0], pos.shape[0], 96
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.ttamm_inbatch_loss_workspace_size(B, Bc, D)), dtype=torch.uint8, device="cuda")
    ttamm._lib.check(lib.ttamm_inbatch_bce_loss(wide_u.data_ptr(), B, 128, wide_p.data_ptr(), Bc, 104, D, 0,
                                                loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                                ttamm._lib.stream_handle(users.device)))
    assert float(loss) == float(ttamm.inbatch_bce_loss(users, pos))


def test_bad_shapes_and_dtypes_raise():
    u = torch.zeros((16, 32), device="cuda")
    with pytest.raises(ValueError, match="one D"):
        ttamm.inbatch_bce_loss(u, torch.zeros((16, 24), device="cuda"))
    with pytest.raises(ValueError, match="row_base"):
        ttamm.inbatch_bce_loss(u, torch.zeros((20, 32), device="cuda"), row_base=8)
    with pytest.raises(ValueError, match="row_base"):
        ttamm.inbatch_bce_loss(u, torch.zeros((20, 32), device="cuda"), row_base=-1)
    with pytest.raises(ValueError, match="float32"):
        ttamm.inbatch_bce_loss(u.double(), torch.zeros((16, 32), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="one D"):
        ttamm.inbatch_bce_loss(u.reshape(-1), torch.zeros((16, 32), device="cuda"))
    with pytest.raises(ValueError, match="multiple of 4"):
        ttamm.inbatch_bce_loss(torch.zeros((16, 10), device="cuda"), torch.zeros((16, 10), device="cuda"))
    with pytest.raises(ValueError, match="multiple of 4"):
        ttamm.inbatch_bce_loss(torch.zeros((16, 132), device="cuda"), torch.zeros((16, 132), device="cuda"))
    with pytest.raises(RuntimeError, match="executes on an MI355X"):
        ttamm.inbatch_bce_loss(u.cpu(), torch.zeros((16, 32)))
