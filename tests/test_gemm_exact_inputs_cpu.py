"""The exact-arithmetic tower problems of tests/exact_inputs.py, checked on the CPU: every case the
GPU test (test_gemm_paths_gpu.test_tower_exact_inputs_bit_exact) runs must satisfy the order-free
precondition, the oracle's own fp32 arithmetic must already reproduce float64 bit for bit on it
(fp32 and the bf16 restatement), and no gradient may be mostly zeros."""

from __future__ import annotations

import copy

import pytest
import torch

import exact_inputs as ex
from oracle import cpu_reference as ref

PAIRS = [(name, R) for name, case in ex.CASES.items() for R in case.rows]


def _oracle(prob: ex.ExactProblem, dtype: torch.dtype, matmul_dtype: str):
    tower = copy.deepcopy(prob.tower).to(dtype)
    tower.matmul_dtype = matmul_dtype
    out = ref.tower_forward(tower, prob.idx, prob.feats.to(dtype), None, training=True)
    out.backward(prob.gy.to(dtype))
    return out.detach(), {n: p.grad for n, p in tower.named_parameters()}


@pytest.mark.parametrize("name,R", PAIRS, ids=[f"{n}-r{r}" for n, r in PAIRS])
def test_exact_inputs_fp32_equals_fp64(name, R):
    case = ex.CASES[name]
    prob = ex.build(case.shape, R, case.recipe)
    out64, g64, pc = ex.reference(prob)
    assert pc.ok, str(pc)
    o32, g32 = _oracle(prob, torch.float32, "fp32")
    o64, gd = _oracle(prob, torch.float64, "fp32")
    assert torch.equal(o64, out64) and torch.equal(o32.double(), out64)
    assert set(g32) == set(g64) == set(gd)
    for n in g64:
        assert torch.equal(gd[n], g64[n]), n  # the oracle in float64 == the GEMM-by-GEMM restatement
        assert g32[n].dtype == torch.float32 and torch.equal(g32[n].double(), g64[n]), n
        nz = float((g64[n] != 0).double().mean())
        assert nz >= 0.9, f"{n}: {nz:.1%} non-zero entries"
    print(f"\n{name} R={R}: {pc}")


@pytest.mark.parametrize("name,R", [p for p in PAIRS if p[0] not in ex.PLANE_CASES],
                         ids=[f"{n}-r{r}" for n, r in PAIRS if n not in ex.PLANE_CASES])
def test_exact_inputs_bf16_restatement_equals_fp64(name, R):
    case = ex.CASES[name]
    prob = ex.build(case.shape, R, case.recipe)
    out64, g64, pc = ex.reference(prob, bf16=True)
    assert pc.ok, str(pc)
    o32, g32 = _oracle(prob, torch.float32, "bf16")
    assert torch.equal(o32.double(), out64)
    assert set(g32) == set(g64)
    for n in g64:
        assert torch.equal(g32[n].double(), g64[n]), n
        nz = float((g64[n] != 0).double().mean())
        assert nz >= 0.9, f"{n}: {nz:.1%} non-zero entries"
    # (where every activation stays below 256 the rounding is the identity and the bf16 result is
    # the fp32 one; it acts at the deeper and wider cases)
    _, g_fp32, _ = ex.reference(prob)
    acts = any(not torch.equal(g_fp32[n], g64[n]) for n in g64)
    print(f"\n{name} R={R}: {pc}; bf16 rounding changes the result: {acts}")
    if name in ("classes", "c4dims"):
        assert acts


def test_lsb_and_precondition_detect_inexact_inputs():
    """The precondition is not vacuous: random fp32 inputs fail it."""
    assert ex._lsb(torch.tensor([3.0, 0.0, -0.75], dtype=torch.float64)) == 0.25
    assert ex._lsb(torch.tensor([4.0, 12.0], dtype=torch.float64)) == 4.0
    case = ex.CASES["narrow"]
    prob = ex.build(case.shape, 129)
    prob.feats = torch.randn(prob.feats.shape, generator=torch.Generator().manual_seed(0))
    _, _, pc = ex.reference(prob)
    assert not pc.ok
