"""The table optimizers compute, bit for bit, what the library computed at the commit before
csrc/optim.hip was split into group.hip / replay.hip / optim.hip (optim_math.h), lost its developer
variants (the scalar-constant replay, the multi-column row update, the piece-sum force switch) and
kept one prepare path (launch_prepare_segs) for one or two towers.

``tests/golden/optim_parent.json`` holds that build's results (recorded results only, written by
tests/golden/make_optim_parent_fixture.py on an MI355X): per case a sha256 over every parameter, both
moments (or momentum buffers) and the step counters, and the losses as float hex strings.

Every case is a FusedTrainStep run built by test_deferred_gpu._run: 13 steps, 3 replay slices, an
lr change at step 6 and (deferred cases) a flush at step 4, on the default Shape() (U = 64, I = 256,
D = 8, B = 32) unless the case says otherwise:

  * replay width: D = 8 (two float4s per replay thread) and D = 12 (one), fast and exact table math;
  * optimizers: coupled Adam, SGD with momentum 0.9, with Nesterov, with momentum 0;
  * eager (dense sweep, side buffers, side scatter) with sparse and with dense ID tables;
  * the one-stream prepare path: overlap=False, and deferred dense ID tables (which never fork);
  * clipping (deferred, dense ID tables): gradient_clip_norm=1.0, which never binds at this shape
    (coefficient 1), and 1e-3, which binds at every step, so the sums of squares, the coefficient
    and the row updates' gradient scaling all reach the digest;
  * padding_idx = 0 with sparse and with dense ID tables;
  * hot rows: B = 128 over U = 4 users, so every user-tower batch holds a row with more than 32
    positions (piece_sum, the long-segment ordering) and one with 17 to 32 (long ordering, direct
    sum) — counted on the CPU before the run."""

from __future__ import annotations

import hashlib
import json
from pathlib import Path

import pytest
import torch

from helpers import Shape, make_problem
from test_deferred_gpu import _batches, _run

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "optim_parent.json"

STEPS, SLICES, LR_CHANGE_AT, FLUSH_AT = 13, 3, 6, 4
# U = 4 is the smallest user count at which _batches' draws (seed 3, B = 128) give both a row above
# 32 positions and one of 17 to 32 (U = 2: 68 / 60, U = 3: 40 / 46 / 42); I = 16 leaves the sampler
# 12 non-positive items per user.  (_batches seeds its own generator and _run draws its batches from
# it, so the ids counted in _hot_row_counts are the ids of the run; were _batches to change, the
# counts are taken again from whatever it draws and the case fails if they no longer qualify.)
HOT = Shape(U=4, I=16, B=128)

# name -> (shape, _run keywords)
CASES = {
    "d8-fast": (Shape(), dict(math="fast")),
    "d8-exact": (Shape(), dict(math="exact")),
    "d12-fast": (Shape(D=12), dict(math="fast")),
    "d12-exact": (Shape(D=12), dict(math="exact")),
    "adam-coupled": (Shape(), dict(coupled=True)),
    "sgd-momentum": (Shape(), dict(sgd=dict(momentum=0.9))),
    "sgd-nesterov": (Shape(), dict(sgd=dict(momentum=0.9, nesterov=True))),
    "sgd-no-momentum": (Shape(), dict(sgd=dict(momentum=0.0))),
    "eager-sparse-id": (Shape(), dict(deferred=False)),
    "eager-dense-id": (Shape(), dict(deferred=False, sparse=False)),
    "no-overlap": (Shape(), dict(overlap=False)),
    "deferred-dense-id": (Shape(), dict(sparse=False)),
    "clip-dense-id": (Shape(), dict(sparse=False, gradient_clip_norm=1.0)),
    "clip-binding-dense-id": (Shape(), dict(sparse=False, gradient_clip_norm=1e-3)),
    "padding-sparse-id": (Shape(padding_idx=0), dict()),
    "padding-dense-id": (Shape(padding_idx=0), dict(sparse=False)),
    "hot-rows": (HOT, dict()),
}


def _digest(tensors: dict) -> str:
    h = hashlib.sha256()
    for name in sorted(tensors):
        t = tensors[name].detach().cpu().contiguous()
        h.update(f"{name}:{tuple(t.shape)}:{t.dtype};".encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def _one(shape, kw) -> dict:
    kw = dict(deferred=True, **kw) if "deferred" not in kw else dict(kw)
    prob = make_problem(shape, seed=21)
    state, losses = _run(prob, STEPS, slices=SLICES, lr_change_at=LR_CHANGE_AT,
                         flush_at=FLUSH_AT if kw["deferred"] else None, **kw)
    torch.cuda.synchronize()
    return {"state": _digest(state), "losses": [float(v).hex() for v in losses]}


def _hot_row_counts(shape) -> list[list[int]]:
    """Positions per user row in each of the run's user-tower batches (the ids _run will draw)."""
    prob = make_problem(shape, seed=21)
    return [torch.bincount(users.cpu(), minlength=shape.U).tolist() for users, _ in _batches(prob, STEPS)]


def run_case(name: str) -> dict:
    shape, kw = CASES[name]
    if name == "hot-rows":
        for k, counts in enumerate(_hot_row_counts(shape)[:3]):
            assert max(counts) > 32, f"batch {k}: no row with more than 32 positions: {counts}"
            assert any(17 <= c <= 32 for c in counts), f"batch {k}: no row with 17 to 32 positions: {counts}"
    out = _one(shape, kw)
    if name == "no-overlap":  # the same run with the prologue on the aux stream
        out["overlap_state"] = _one(shape, dict(kw, overlap=True))["state"]
    return out


def test_fixture_covers_every_case():
    recorded = json.loads(GOLDEN.read_text())["cases"]
    assert sorted(recorded) == sorted(CASES)
    # the one-stream and the aux-stream prologue agreed at the parent commit already
    assert recorded["no-overlap"]["overlap_state"] == recorded["no-overlap"]["state"] == recorded["d8-fast"]["state"]
    # sensitivity: the digest sees the table arithmetic (fast and exact part within a few ulp)
    assert recorded["d8-fast"]["state"] != recorded["d8-exact"]["state"]
    assert recorded["d12-fast"]["state"] != recorded["d12-exact"]["state"]
    # the binding clip norm scaled the gradients: neither the unclipped run's bits nor its later losses
    assert recorded["clip-binding-dense-id"]["state"] != recorded["deferred-dense-id"]["state"]
    assert recorded["clip-binding-dense-id"]["losses"][1:] != recorded["deferred-dense-id"]["losses"][1:]


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_parent_commit(name):
    want = json.loads(GOLDEN.read_text())["cases"][name]
    got = run_case(name)
    print(f"\n{name}: got {got} parent {want}")
    assert got == want
