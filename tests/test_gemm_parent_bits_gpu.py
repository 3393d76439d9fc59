"""The tower GEMMs compute, bit for bit, what the library computed at the commit before
csrc/gemm.hip lost its developer variants and dead code and was rebuilt on one launcher, one epilogue
switch, one weight-gradient kernel table, one epilogue geometry (EpiGeom) and one bias rule (bias4_of).

``tests/golden/gemm_parent.json`` holds that build's results (recorded results only, written by
tests/golden/make_gemm_parent_fixture.py on an MI355X: the weight gradients' rows per split follow
the device's CU count and the kernels' occupancy): per case a sha256 over the result tensors and
the losses as float hex strings.

The exact-arithmetic tests (test_gemm_paths_gpu.py) are independent of the summation order and the
oracle tests hold 1e-5; these cases pin the summation order of every kernel family on seeded
``randn`` inputs drawn on the CPU:

  * tower under autograd (build_tower_encoder, train-mode forward + backward(gy); the digest covers
    the output and every parameter gradient) in four modes — split-bf16 (default),
    TTAMM_FP32_MFMA=exact, bf16 towers, bf16 + exact — over F = 12 .. 100 (1 to 7 k-tiles of 16:
    every entry and exit of the six-step A-operand ring, 12 and 100 ragged), the tile widths and
    weight-gradient classes, the ones column alone in an M tile, one-row and 127-row calls, three
    row splits with a ragged last one, and a GELU layer with drawn dropout (pre, mask_out, keep_mask);
  * the fused step, two steps at lr 1e-3 (the digest covers every parameter, both moments and the
    losses): the generic-gate epilogues, the drawn dropout stream, feature planes, bf16 towers."""

from __future__ import annotations

import hashlib
import json
import os
from pathlib import Path

import pytest
import torch

import exact_inputs as ex
import ttamm
from helpers import Shape, make_problem, named_optimizer_state

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_parent.json"

MODES = {"split": (False, False), "exact": (True, False), "bf16": (False, True), "bf16-exact": (True, True)}

# name -> (F, hidden, D, rows of each tower call, Shape overrides)
TOWERS = {f"ring-f{F}": (F, (24,), 12, (129,), {}) for F in (12, 32, 48, 64, 80, 96, 100)}
TOWERS.update({
    "classes": (37, (100, 160, 200), 12, (257,), {}),
    "class3": (40, (256,), 32, (129,), {}),
    "c2dims": (605, (192,), 96, (300,), {}),
    "ones-tile": (128, (32,), 16, (129,), {}),
    "one-row": (40, (64,), 32, (1, 127), {}),
    "split-k": (40, (64,), 32, (2100,), {}),
    "gelu-drop": (37, (100, 24), 12, (257,), {"activation": "gelu", "dropout": 0.3}),
})


def _step_cases() -> dict:
    """name -> (shape, exact, generic gate, _run_engine keywords)"""
    from test_gemm_paths_gpu import PLANE_SHAPES, TILE_SHAPES, _step_shapes
    from test_step_parity_gpu import GATE_SHAPES

    drop = Shape(dropout=0.3, hidden_dims=(100, 20))
    drawn = dict(masks=False, seed=20240607)
    cases = {
        "gate-w256": (TILE_SHAPES[2], False, False, {}),
        "gate-w256-exact": (TILE_SHAPES[2], True, False, {}),
        "generic-gate-d96": (GATE_SHAPES[2], False, True, {}),
        "drawn-dropout": (drop, False, False, drawn),
        "drawn-dropout-exact": (drop, True, False, drawn),
    }
    for name in ("f37", "f128", "f40-h256"):
        cases[f"planes-{name}"] = (PLANE_SHAPES[name][0], False, False, {"feature_planes": True})
    for name in ("bf16-tiny", "bf16-odd"):
        cases[name] = (_step_shapes()[name][0], False, False, {})
    return cases


# (kind, name, mode)
CASES = [("tower", name, mode) for name in TOWERS for mode in MODES] + [("step", name, "") for name in _step_cases()]


def case_id(c) -> str:
    kind, name, mode = c
    return f"{kind}-{name}" + (f"-{mode}" if mode else "")


def _digest(tensors: dict) -> str:
    h = hashlib.sha256()
    for name in sorted(tensors):
        t = tensors[name].detach().cpu().contiguous()
        h.update(f"{name}:{tuple(t.shape)}:{t.dtype};".encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


class _Env:
    """TTAMM_FP32_MFMA / TTAMM_GENERIC_GATE for one case (both are read at every launch or when the
    engine is built), restored afterwards."""

    NAMES = ("TTAMM_FP32_MFMA", "TTAMM_GENERIC_GATE")

    def __init__(self, exact: bool, generic: bool):
        self.want = {"TTAMM_FP32_MFMA": "exact" if exact else None, "TTAMM_GENERIC_GATE": "1" if generic else None}

    def __enter__(self):
        self.before = {n: os.environ.pop(n, None) for n in self.NAMES}
        for n, v in self.want.items():
            if v is not None:
                os.environ[n] = v

    def __exit__(self, *exc):
        for n in self.NAMES:
            os.environ.pop(n, None)
            if self.before[n] is not None:
                os.environ[n] = self.before[n]


def _run_tower(name: str, mode: str) -> dict:
    F, hidden, D, rows, over = TOWERS[name]
    exact, bf16 = MODES[mode]
    shape = Shape(**{**ex._shape(F, hidden, D).__dict__, **over, "matmul_dtype": "bf16" if bf16 else "fp32"})
    out = {}
    for R in rows:
        I = R  # every ID row is looked up once: the table gradient's scatter adds have no order to depend on
        tower = make_problem(Shape(**{**shape.__dict__, "I": I}), steps=0).model.item_encoder  # seeded default init
        g = torch.Generator(device="cpu").manual_seed((F * 1000003 + D) * 1009 + R)
        feats = torch.randn((R, F), generator=g)
        gy = torch.randn((R, shape.P), generator=g)
        idx = torch.randperm(I, generator=g)
        enc = ttamm.build_tower_encoder(shape.tower_cfg(), num_embeddings=I, feature_dim=F, device="cuda")
        res = enc.load_state_dict({k: v.cuda() for k, v in tower.state_dict().items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        enc.train()
        torch.manual_seed(20240607 + R)  # the dropout stream's key comes from torch's global generator
        with _Env(exact, False):
            y = enc({"indices": idx.cuda(), "features": feats.cuda()})
            y.backward(gy.cuda())
            torch.cuda.synchronize()
        tensors = {"out": y, **{f"grad.{n}": p.grad for n, p in enc.named_parameters()}}
        assert all(t is not None and not t.is_sparse for t in tensors.values())
        out[f"R{R}"] = _digest(tensors)
    return out


def _run_step(name: str) -> dict:
    from test_gemm_paths_gpu import _run_engine

    shape, exact, generic, kw = _step_cases()[name]
    prob = make_problem(shape, steps=2)
    with _Env(exact, generic):
        model, opts, losses, _ = _run_engine(prob, lr=1e-3, betas=(0.9, 0.999), **kw)
        torch.cuda.synchronize()
    tensors = {f"param.{n}": p for n, p in model.state_dict().items()}
    for n, st in named_optimizer_state(model, opts).items():
        tensors[f"exp_avg.{n}"] = st["exp_avg"]
        tensors[f"exp_avg_sq.{n}"] = st["exp_avg_sq"]
    return {"state": _digest(tensors),
            "losses": [{k: float(v).hex() for k, v in sorted(step.items())} for step in losses]}


def run_case(c) -> dict:
    kind, name, mode = c
    return _run_tower(name, mode) if kind == "tower" else _run_step(name)


def test_fixture_covers_every_case():
    recorded = json.loads(GOLDEN.read_text())["cases"]
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)
    # every mode reached its own kernels when the fixture was written: the split-bf16, fp32-MFMA and
    # bf16 arithmetic never share their bits, nor do the default and the exact run of a step.  (The two
    # bf16 kernels sum the same exact bf16 products and agree at short K; they part where K spans
    # several k-tiles, so somewhere.)
    bf16_parted = 0
    for name in TOWERS:
        got = {m: json.dumps(recorded[case_id(("tower", name, m))], sort_keys=True) for m in MODES}
        assert len({got["split"], got["exact"], got["bf16"]}) == 3 and got["bf16-exact"] not in (got["split"], got["exact"]), name
        bf16_parted += got["bf16"] != got["bf16-exact"]
    assert bf16_parted > 0
    for a, b in (("gate-w256", "gate-w256-exact"), ("drawn-dropout", "drawn-dropout-exact")):
        assert recorded[case_id(("step", a, ""))]["state"] != recorded[case_id(("step", b, ""))]["state"]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_bits_equal_the_parent_commit(c):
    want = json.loads(GOLDEN.read_text())["cases"][case_id(c)]
    got = run_case(c)
    print(f"\n{case_id(c)}: got {got} parent {want}")
    assert got == want
