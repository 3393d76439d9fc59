"""The four in-batch ops compute, bit for bit, what the library computed at the commit before
csrc/inbatch.hip was rebuilt from shared pieces (one row-fragment load, one tile stage, one score
block, one set of element arithmetic, one host path) and lost its two developer kernel variants.

``tests/golden/inbatch_parent.json`` holds that build's results (recorded results only, written by
tests/golden/make_inbatch_parent_fixture.py): per case the loss sum as a float64 hex string and a
sha256 of dU and of dP.  Ops: ttamm_inbatch_bce, ttamm_inbatch_bce_loss, ttamm_inbatch_softmax,
ttamm_inbatch_softmax_loss, and ttamm_inbatch_bce under TTAMM_FP32_MFMA=exact (the fp32-MFMA
inbatch_kernel).

Shapes (B, Bc, D, row_base): those tests/test_inbatch_loss_gpu.py and tests/test_inbatch_softmax_gpu.py
argue for — every D class, a ragged D, the second 128-row and 256-row blocks with two live rows,
ragged last splits, multi-tile splits, a label in the last partial tile — and the softmax ops
additionally at temperature 0.25 and 0.02.  Inputs come from a CPU generator seeded from the
shape, so the fixture does not depend on the device's random numbers."""

from __future__ import annotations

import hashlib
import json
import os
from pathlib import Path

import pytest
import torch

import ttamm

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "inbatch_parent.json"

SHAPES = [
    (1, 1, 4, 0),
    (64, 64, 64, 0),
    (77, 77, 12, 0),
    (130, 130, 32, 0),
    (258, 258, 32, 0),
    (300, 300, 96, 0),
    (200, 900, 128, 450),
    (33, 700, 96, 667),
    (40, 50000, 32, 49000),
    (2100, 2100, 64, 0),
]
SOFTMAX_ONLY = [((300, 300, 96, 0), 0.25), ((200, 900, 64, 450), 0.02)]
OPS = ("bce", "bce_loss", "softmax", "softmax_loss", "bce_exact")

# (op, shape, temperature)
CASES = [(op, s, 1.0) for op in OPS for s in SHAPES]
CASES += [(op, s, t) for op in ("softmax", "softmax_loss") for s, t in SOFTMAX_ONLY]


def case_id(c) -> str:
    op, (B, Bc, D, row_base), t = c
    return f"{op}-B{B}-Bc{Bc}-D{D}-base{row_base}" + ("" if t == 1.0 else f"-t{t}")


def inputs(shape):
    """randn x scale, the own positive += 0.5 x user, drawn on the CPU."""
    B, Bc, D, row_base = shape
    g = torch.Generator(device="cpu").manual_seed((((B * 1000003 + Bc) * 1009 + D) * 1000003 + row_base) % (1 << 62))
    scale = 0.5 if D <= 16 else 0.3
    users = torch.randn((B, D), generator=g) * scale
    pos = torch.randn((Bc, D), generator=g) * scale
    pos[row_base:row_base + B] += 0.5 * users
    return users.cuda(), pos.cuda()


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(c) -> dict:
    """One op on one case: {"loss": float64 hex, and with gradients "dU" / "dP": sha256}."""
    op, shape, t = c
    users, pos = inputs(shape)
    row_base = shape[3]
    if op == "bce_loss":
        return {"loss": float(ttamm.inbatch_bce_loss(users, pos, row_base=row_base)).hex()}
    if op == "softmax_loss":
        return {"loss": float(ttamm.inbatch_softmax_loss(users, pos, row_base=row_base, temperature=t)).hex()}
    if op == "softmax":
        loss, du, dp = ttamm.inbatch_softmax(users, pos, row_base=row_base, temperature=t)
    else:
        before = os.environ.pop("TTAMM_FP32_MFMA", None)
        if op == "bce_exact":
            os.environ["TTAMM_FP32_MFMA"] = "exact"  # read at every launch
        try:
            loss, du, dp = ttamm.inbatch_bce(users, pos, row_base=row_base)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("TTAMM_FP32_MFMA", None)
            if before is not None:
                os.environ["TTAMM_FP32_MFMA"] = before
    return {"loss": float(loss).hex(), "dU": _sha(du), "dP": _sha(dp)}


def test_fixture_covers_every_case():
    recorded = json.loads(GOLDEN.read_text())["cases"]
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)
    # the fp32-MFMA kernel was reached when the fixture was written: its bits are not the default's
    differ = sum(recorded[case_id(("bce_exact", s, 1.0))] != recorded[case_id(("bce", s, 1.0))] for s in SHAPES)
    assert differ > 0


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_bits_equal_the_parent_commit(c):
    want = json.loads(GOLDEN.read_text())["cases"][case_id(c)]
    got = run_case(c)
    print(f"\n{case_id(c)}: got {got} parent {want}")
    assert got == want
