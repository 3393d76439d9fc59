"""The fused gate kernels launched in whole slab rounds (csrc/gate.hip gate_blocks, gate_plan.h)
change no bit: which wave owns a slab enters no result.

Every case runs three one-process training steps and is compared bit for bit with what the
library computed at the commit before the change: ``tests/golden/gate_rounds_parent.json`` holds
that build's losses and a sha256 of every parameter and optimizer-state tensor (recorded results
only, written by tests/golden/make_gate_rounds_fixture.py).

Tiny tables (U = 300, I = 2000), F = 37, gated fusion, mimic on, dropout on with injected masks,
N = 5 sampled negatives unless the case says otherwise.  The step's workspace is filled with 0xFF
bytes (NaN as a float) past its zeroed row-grouping scratch before the first step, so a read of a
row that no block wrote could not go unnoticed (the fixture's maker checked that the parent build
computes the same on a zeroed workspace).

Shapes (16-row slabs, 8 waves a block at D <= 96, 4 at D = 128; 2048 slabs are one round on the
MI355X's 256 CUs -- the device's CU count enters no expected value):
  B = 3              partial slabs, fewer slabs than one block's waves
  B = 50
  B = 300, N = 20    towers of 19 and 394 slabs
  B = 4680           293 + 1755 = 2048 slabs: the last one-round count (each tower's slabs are
                     rounded up on their own, so 7 B = 32,767 rows is already one slab past it)
  B = 4681, 4682     7 B = 32,767 and 32,774 rows, no multiple of 16: two rounds
  B = 9400           three rounds
  D = 64, 32, 128    at B = 50 and B = 4682 (D = 128: 4-wave blocks, G2 from global memory)
and the readers of t | a and aug at B = 50: mimic off, in-batch negatives with N = 2 on top,
category alignment, the one-stream step, gradient clipping, and one compute_loss pass after the
steps (its loss is in the fixture).
"""

from __future__ import annotations

import hashlib
import json
from dataclasses import dataclass, field
from pathlib import Path

import pytest
import torch

from helpers import LOSS_WEIGHTS, Shape, make_problem

GOLDEN = Path(__file__).resolve().parent / "golden" / "gate_rounds_parent.json"
STEPS = 3
U, I, F = 300, 2000, 37
NCAT = 7


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    N: int = 5
    D: int = 96
    H: int = 192
    mimic: bool = True
    dense_id: bool = False            # dense ID tables updated every step (what clipping needs)
    cal: bool = False                 # category alignment
    eval_pass: bool = False           # a compute_loss pass after the steps
    engine: dict = field(default_factory=dict, hash=False, compare=False)  # FusedTrainStep keywords


CASES = [
    Case("B3", 3),
    Case("B50", 50, eval_pass=True),
    Case("B300-N20", 300, N=20),
    Case("B4680", 4680),
    Case("B4681", 4681),
    Case("B4682", 4682),
    Case("B9400", 9400),
    Case("D64-B50", 50, D=64, H=160),
    Case("D64-B4682", 4682, D=64, H=160),
    Case("D32-B50", 50, D=32, H=160),
    Case("D32-B4682", 4682, D=32, H=160),
    Case("D128-B50", 50, D=128, H=160),
    Case("D128-B4682", 4682, D=128, H=160),
    Case("mimic-off", 50, mimic=False),
    Case("in-batch-N2", 50, N=2, engine={"in_batch_negatives": True}),
    Case("category-alignment", 50, cal=True),
    Case("one-stream", 50, engine={"overlap": False}),
    Case("clipped", 50, dense_id=True, engine={"gradient_clip_norm": 0.05}),
]


def shape_of(c: Case) -> Shape:
    return Shape(U=U, I=I, F=F, H=c.H, D=c.D, B=c.B, N=c.N, hidden_dims=(c.H,), mimic=c.mimic, sparse=not c.dense_id)


def categories() -> torch.Tensor:
    return (torch.arange(I) * 5 + 3) % NCAT


def scratch_head_bytes(c: Case) -> int:
    """The workspace's zero-once head (step.hip plan_scratch): three ints per table row for each
    tower's row grouping (and per category with alignment on), then one counter; every piece starts
    at a multiple of 256 bytes, and so do the activations after it."""
    off = 0
    for n in [3 * U * 4, 3 * I * 4] + ([3 * NCAT * 4] if c.cal else []) + [4]:
        off = -(-off // 256) * 256 + n
    return -(-off // 256) * 256


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def state_digests(model, opts) -> dict[str, str]:
    from helpers import named_optimizer_state

    out = {n: digest(p) for n, p in model.named_parameters()}
    for n, st in named_optimizer_state(model, opts).items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"{n}.{k}"] = digest(st[k])
    return out


def run_case(c: Case, poison: bool = True) -> dict:
    """Three steps of the one-process step at case c: the losses and the state's digests."""
    import ttamm
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    prob = make_problem(shape_of(c), steps=STEPS, seed=91)
    model = ttamm_model_from(prob)
    opts = ttamm_optimizers(model)
    kw = dict(c.engine)
    if c.cal:
        kw.update(item_category_tensor=categories().cuda(), major_category_id=0)
    if c.dense_id:
        kw.update(deferred_adamw=False)
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=c.N, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=c.B, **kw)
    if poison:
        head = scratch_head_bytes(c)
        assert head < eng.ws_bytes
        eng.workspace[head:].fill_(0xFF)
    losses = []
    for (users, pos, neg, um, im) in prob.batches:
        eng.step(users.cuda(), pos.cuda(), neg.cuda().reshape(-1),
                 keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})
        losses.append({k: float(v) for k, v in eng.last_losses().items()})
    eng.finish()
    torch.cuda.synchronize()
    out = {"losses": losses, "state": state_digests(model, opts)}
    if c.eval_pass:  # the forward-only pass (its workspace is torch.empty) on the trained model
        negs = [b[2] for b in prob.batches]
        out["eval_loss"] = float(ttamm.compute_loss(
            model, [(b[0], b[1]) for b in prob.batches], criterion=torch.nn.BCEWithLogitsLoss(),
            negatives_per_positive=c.N, num_items=I, user_positive_items=prob.positives,
            user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(), device="cuda",
            batch_hook=lambda step, users, pos: negs[step], seed=5))
    return out


@pytest.fixture(scope="module")
def golden() -> dict:
    return json.loads(GOLDEN.read_text())["cases"]


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(c.name for c in CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_step_is_bit_equal_to_the_parent(c, golden):
    got, want = run_case(c), golden[c.name]
    print(f"\n{c.name}: losses {got['losses'][-1]} eval {got.get('eval_loss')}")
    for l in got["losses"]:
        assert all(v == v for v in l.values()), l  # no NaN from the poisoned workspace
    assert got["losses"] == want["losses"]
    assert got.get("eval_loss") == want.get("eval_loss")
    assert got["state"].keys() == want["state"].keys()
    bad = [k for k in want["state"] if got["state"][k] != want["state"][k]]
    assert not bad, bad
