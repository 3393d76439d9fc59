"""The backward's tail on the one-process step: the MLP dgrad's prefetched mask rows and the slab
reduce fused with the dense AdamW update (kernels.h WgradTail) change no bit.

The step with the aux stream and without clipping (FusedTrainStep's default) runs the fused tail;
``overlap=False`` and a clipped step keep the stand-alone reduce and dense_adam_kernel.  Every
case is compared bit for bit with what the library computed at the commit before the change:
``tests/golden/backward_tail_parent.json`` holds that build's losses and a sha256 of every
parameter and optimizer-state tensor after three steps (recorded results only, written by
tests/golden/make_backward_tail_fixture.py).

Shapes: R_user + R_item not a multiple of the 128-row tile (B = 50, N = 5), a k tail in layer 1
(F = 37), a partial N tile in the dgrad (H = 192 / 160 over 96-wide and 192-wide tiles),
D = 96 / 64 (the dgrad's K), dropout on with injected masks, and a sweep of B that puts the split
counts of both weight-gradient tile classes below, at and above the reduce's load-batch depth
(16), with counts that are no multiple of it.
"""

from __future__ import annotations

import hashlib
import json
from pathlib import Path

import pytest
import torch

from helpers import Shape, make_problem

GOLDEN = Path(__file__).resolve().parent / "golden" / "backward_tail_parent.json"
STEPS = 3
DEPTH = 16  # gemm.hip kWgradReduceDepth, optim.hip kTailDepth
N_NEG = 5

# (B, F, H, D)
CASES = [
    (50, 37, 192, 96),
    (50, 37, 160, 64),
    (16, 37, 192, 96),
    (200, 37, 192, 96),
    (1024, 37, 192, 96),
    (1024, 37, 160, 64),
    (2048, 37, 192, 96),
    (3000, 37, 192, 96),
]
SWEEP = [c for c in CASES if c[2:] == (192, 96)]


def case_id(c) -> str:
    return "B%d-F%d-H%d-D%d" % c


def shape_of(c, sparse: bool = True) -> Shape:
    B, F, H, D = c
    return Shape(U=300, I=2000, F=F, H=H, D=D, B=B, N=N_NEG, hidden_dims=(H,), sparse=sparse)


# ---- split counts (host arithmetic; no device) -------------------------------------------------
def wgrad_class(m_out: int) -> int:
    """gemm.hip wgrad_class: 0 = 96-wide tiles, 1 = 192, 2 = 128, 3 = multiples of 256."""
    if m_out <= 96:
        return 0
    pad = lambda bn: -(-m_out // bn) * bn  # noqa: E731
    best, bp = 1, pad(192)
    if pad(256) < bp:
        best, bp = 3, pad(256)
    if pad(128) < bp:
        best, bp = 2, pad(128)
    return best


def rows_per_split(shapes, slots: int) -> dict[int, int]:
    """gemm.hip wgrad_rows_per_split for (R, M, N) problems with `slots` resident blocks per class."""
    us_per_row = (0.11, 0.14, 0.12, 0.12)
    tile_n = (96, 192, 128, 128)
    out = {}
    for c in range(4):
        best, best_cost = 512, -1.0
        for r in range(128, 1025, 32):
            tiles, slab = 0, 0.0
            for (R, M, N) in shapes:
                if R <= 0 or wgrad_class(M) != c:
                    continue
                splits = -(-R // r)
                tiles += -(-(N + 1) // 128) * -(-M // tile_n[c]) * splits
                slab += 2.0 * 4.0 * splits * M * (N + 1)
            if tiles == 0:
                break
            cost = -(-tiles // slots) * r * us_per_row[c] + slab / 5.0e6
            if best_cost < 0.0 or cost < best_cost:
                best_cost, best = cost, r
        out[c] = best
    return out


def split_counts(c, slots: int) -> dict[int, set[int]]:
    """{tile class: the split counts of its weight gradients} for one case (gated fusion, Hg = D)."""
    B, F, H, D = c
    shapes = []
    for R in (B, B * (1 + N_NEG)):
        shapes += [(R, D, D), (R, D, 2 * D), (R, D, H), (R, H, F)]  # gate.2, gate.0, layer 2, layer 1
    rps = rows_per_split(shapes, slots)
    out: dict[int, set[int]] = {}
    for (R, M, N) in shapes:
        out.setdefault(wgrad_class(M), set()).add(-(-R // rps[wgrad_class(M)]))
    return out


def test_sweep_split_counts_straddle_the_load_batch_depth():
    """Both tile classes see split counts below, at and above DEPTH and one that is no multiple of it.
    The narrow class's rows per split depend on how many of its blocks the device holds (gemm.hip
    wgrad_slots): three per CU on the MI355X's 256 CUs (156 VGPRs, 52 KB of LDS per block); the
    sweep holds from there up."""
    for slots in (256 * 3, 256 * 4, 256 * 8):
        seen: dict[int, set[int]] = {}
        for c in SWEEP:
            for cls, counts in split_counts(c, slots).items():
                seen.setdefault(cls, set()).update(counts)
        assert set(seen) == {0, 1}, seen
        for cls, counts in seen.items():
            assert any(s < DEPTH for s in counts), (cls, counts)
            assert DEPTH in counts, (cls, counts)
            assert any(s > DEPTH and s % DEPTH == 0 for s in counts), (cls, counts)
            assert any(s > DEPTH and s % DEPTH != 0 for s in counts), (cls, counts)


# ---- the recorded runs --------------------------------------------------------------------------
def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def state_digests(model, opts) -> dict[str, str]:
    from helpers import named_optimizer_state

    out = {n: digest(p) for n, p in model.named_parameters()}
    for n, st in named_optimizer_state(model, opts).items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"{n}.{k}"] = digest(st[k])
    return out


def run_case(c, sparse: bool = True, **kw) -> dict:
    """Three steps of the one-process step at case c: the losses and the state's digests."""
    from gpu_helpers import run_ttamm

    prob = problem(c, sparse)
    model, opts, losses = run_ttamm(prob, steps=STEPS, **kw)
    torch.cuda.synchronize()
    return {"losses": [{k: float(v) for k, v in l.items()} for l in losses], "state": state_digests(model, opts)}


_problems: dict = {}


def problem(c, sparse: bool = True):
    if (c, sparse) not in _problems:
        _problems[c, sparse] = make_problem(shape_of(c, sparse), steps=STEPS, seed=77)
    return _problems[c, sparse]


@pytest.fixture(scope="module")
def golden() -> dict:
    return json.loads(GOLDEN.read_text())["cases"]


def _assert_same(got: dict, want: dict) -> None:
    assert got["losses"] == want["losses"]
    assert got["state"].keys() == want["state"].keys()
    bad = [k for k in want["state"] if got["state"][k] != want["state"][k]]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fused_tail_step_is_bit_equal_to_the_parent(c, golden):
    _assert_same(run_case(c), golden[case_id(c)])


TWIN_CASES = [CASES[0], CASES[5], CASES[7]]
# dense ID tables updated every step: clipping needs dense gradients, and the step keeps its aux stream
DENSE_ID = {"sparse": False, "deferred_adamw": False}


def dense_id_key(c) -> str:
    return case_id(c) + "/dense-id"


# Twins that run the stand-alone reduce (with its deeper load batches) and dense_adam_kernel.  On
# the parent both were bit-equal to the step they are compared with, in every case
# (make_backward_tail_fixture.py records that as "twins_equal"): the one-stream step
# (overlap=False) to the default step, and the clipped step with a coefficient of 1.0
# (gradient_clip_norm=1e30) to the unclipped step over dense ID tables.
@pytest.mark.gpu
@pytest.mark.parametrize("c", TWIN_CASES, ids=case_id)
def test_one_stream_twin_is_bit_equal(c, golden):
    _assert_same(run_case(c, overlap=False), golden[case_id(c)])


@pytest.mark.gpu
@pytest.mark.parametrize("c", TWIN_CASES, ids=case_id)
def test_clipped_twin_with_coefficient_one_is_bit_equal(c, golden):
    fused = run_case(c, **DENSE_ID)
    _assert_same(fused, golden[dense_id_key(c)])
    _assert_same(run_case(c, **DENSE_ID, gradient_clip_norm=1e30), fused)


@pytest.mark.gpu
def test_poisoned_step_leaves_parameters_and_moments_untouched():
    """An out-of-range id: the fused tail writes the gradients and no parameter, m or v."""
    import ttamm
    from gpu_helpers import ttamm_model_from, ttamm_optimizers
    from helpers import LOSS_WEIGHTS

    c = CASES[0]
    prob = problem(c)

    def engine():
        model = ttamm_model_from(prob)
        opts = ttamm_optimizers(model)
        eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=N_NEG, positives=prob.positives,
                                   user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                                   loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B)
        return model, opts, eng

    def step(eng, k, bad):
        users, pos, neg, um, im = prob.batches[k]
        users = users.clone()
        if bad:
            users[7] = prob.shape.U + 11
        eng.step(users.cuda(), pos.cuda(), neg.cuda().reshape(-1),
                 keep_masks={"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]})

    # the state after one good step (so the moments are not all zero) ...
    m1, o1, e1 = engine()
    step(e1, 0, False)
    e1.finish()
    want = state_digests(m1, o1)
    # ... is the state after that step, a poisoned one and a good one (skipped too)
    m2, o2, e2 = engine()
    step(e2, 0, False)
    step(e2, 1, True)
    step(e2, 2, False)
    with pytest.raises(IndexError):
        e2.finish()
    torch.cuda.synchronize()
    assert state_digests(m2, o2) == want
