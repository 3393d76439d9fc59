"""Workspace sizes of every entry that runs a tower, over a small descriptor matrix.

All five size queries lay their towers out with one planner (csrc/tower.hip plan_tower), so they
must agree with each other (a forward-only workspace is no larger than the forward + backward
one) and with the library as it was before the planner was shared: the buffer set per entry is
unchanged, so a size may move only by the unpadded tail of the last 256-byte aligned take.  The
earlier library's sizes are recorded results (tests/golden/tower_workspace_parent.json, written
by tests/golden/make_tower_workspace_fixture.py).

Host logic only: the size queries dereference no pointer, so the descriptors carry fake non-null
pointers (as tests/test_eval_loss_cpu.py does) and the library loads without a GPU.
"""

from __future__ import annotations

import ctypes
import itertools
import json
from pathlib import Path

import pytest

from ttamm import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "tower_workspace_parent.json"
FAKE = 4096  # never dereferenced
ROWS = (1, 16)  # n of the single-tower entries, B of the step / eval-loss entries
NUM_NEG = 2
TABLE_ROWS = 50
UNIT = 256  # Arena alignment

QUERIES = ("train_step", "eval_loss", "eval_loss_inbatch", "tower_train", "tower_forward")

FUSIONS = {"identity": _lib.FUSION_IDENTITY, "sum": _lib.FUSION_SUM, "gated": _lib.FUSION_GATED,
           "concat": _lib.FUSION_CONCAT}
ACTS = {"relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}
# (matmul_bf16, bf16 feature rows given); D = Hg = 128 is a gate16 width, D = 8 a generic one
PRECISIONS = {"fp32": (0, False), "bf16": (1, False), "bf16feat": (1, True)}
WIDTHS = (8, 128)
FEATS = (20, 21)  # 21: a first layer with in_features % 4 != 0


# (activation, dropout, max_norm, mimic, F): every pair of these five two-valued switches takes all
# four of its value pairs within the four rows, so the matrix stays small
SWITCHES = (("relu", 0.0, 0, 0, 20), ("relu", 0.1, 1, 1, 21), ("gelu", 0.0, 1, 0, 21), ("gelu", 0.1, 0, 1, 20))


def _cases():
    """What shapes a tower's buffers (fusion, layers, precision, width) in full product, crossed
    with the four rows of SWITCHES."""
    out = []
    for fusion, nl, prec, D, (act, drop, mn, mimic, F) in itertools.product(
            FUSIONS, (0, 1, 2), PRECISIONS, WIDTHS, SWITCHES):
        out.append(dict(fusion=fusion, n_linear=nl, act=act, dropout=drop, max_norm=mn, mimic=mimic, prec=prec,
                        D=D, F=F if nl else FEATS[0]))  # no first layer: one feature width
    return out


def case_id(c: dict) -> str:
    return (f"{c['fusion']}-L{c['n_linear']}-{c['act']}-p{c['dropout']}-mn{c['max_norm']}-mim{c['mimic']}-"
            f"{c['prec']}-D{c['D']}-F{c['F']}")


CASES = _cases()


def _linear(s: _lib.Linear, fin: int, fout: int) -> None:
    s.weight = s.bias = FAKE
    s.weight_exp_avg = s.weight_exp_avg_sq = s.bias_exp_avg = s.bias_exp_avg_sq = FAKE
    s.in_features, s.out_features = fin, fout


def fill_tower(t: _lib.Tower, c: dict) -> None:
    """A descriptor shaped as validate_tower wants it (sum / gated: the feature encoder ends D wide)."""
    D, nl = c["D"], c["n_linear"]
    t.id.weight = t.id.exp_avg = t.id.exp_avg_sq = FAKE
    t.id.rows, t.id.dim = TABLE_ROWS, D
    if c["max_norm"]:
        t.id.max_norm = 1.0
        t.id.optimizer = _lib.OPT_DENSE
    if c["mimic"]:
        t.mimic.weight = t.mimic.exp_avg = t.mimic.exp_avg_sq = FAKE
        t.mimic.rows, t.mimic.dim = TABLE_ROWS, D
        t.mimic.optimizer = _lib.OPT_DENSE
    t.fusion = FUSIONS[c["fusion"]]
    bf16, feat16 = PRECISIONS[c["prec"]]
    t.matmul_bf16 = bf16
    F = c["F"] if nl > 0 or c["fusion"] == "concat" else D
    t.features = FAKE
    t.feat_dim = F
    t.feat_ld = (F + 3) // 4 * 4
    if feat16:
        t.features_bf16 = FAKE
        t.feat_bf16_ld = (F + 7) // 8 * 8
    t.dropout = c["dropout"]
    t.activation = ACTS[c["act"]]
    t.n_linear = nl
    widths = [F] + ([64] if nl == 2 else []) + ([D] if nl else [])
    for i in range(nl):
        _linear(t.linear[i], widths[i], widths[i + 1])
    if c["fusion"] == "gated":
        _linear(t.gate[0], 2 * D, D)
        _linear(t.gate[1], D, D)
    elif c["fusion"] == "concat":
        _linear(t.gate[0], D + widths[-1], D)


def query_sizes(lib, c: dict, rows: int) -> list[int]:
    """The five size queries (QUERIES order) for one tower descriptor used as both towers."""
    args = _lib.StepArgs()
    fill_tower(args.user, c)
    fill_tower(args.item, c)
    args.mimic_enabled = c["mimic"]
    args.b.batch = rows
    args.b.num_neg = NUM_NEG
    tower = _lib.Tower()
    fill_tower(tower, c)
    return [
        lib.ttamm_train_step_workspace_size(ctypes.byref(args)),
        lib.ttamm_eval_loss_workspace_size(ctypes.byref(args)),
        lib.ttamm_eval_loss_inbatch_workspace_size(ctypes.byref(args)),
        lib.ttamm_tower_train_workspace_size(ctypes.byref(tower), rows),
        lib.ttamm_tower_forward_workspace_size(ctypes.byref(tower), rows),
    ]


@pytest.fixture(scope="module")
def sizes() -> dict:
    lib = _lib.load()
    return {case_id(c): {n: dict(zip(QUERIES, query_sizes(lib, c, n))) for n in ROWS} for c in CASES}


@pytest.fixture(scope="module")
def parent() -> dict:
    return json.loads(GOLDEN.read_text())


def test_matrix_covers_what_selects_a_buffer():
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for key, vals in (("fusion", FUSIONS), ("n_linear", (0, 1, 2)), ("act", ACTS), ("dropout", (0.0, 0.1)),
                      ("max_norm", (0, 1)), ("mimic", (0, 1)), ("prec", PRECISIONS), ("D", WIDTHS)):
        assert {c[key] for c in CASES} == set(vals)
    assert any(c["F"] % 4 for c in CASES if c["n_linear"] > 0)


def test_forward_only_tower_is_no_larger_than_forward_plus_backward(sizes):
    bad = []
    for c in CASES:
        for n in ROWS:
            s = sizes[case_id(c)][n]
            # identity fusion: the backward adds nothing, so equality within one Arena unit
            slack = UNIT if c["fusion"] == "identity" else 0
            if s["tower_forward"] > s["tower_train"] + slack:
                bad.append((case_id(c), n, s["tower_forward"], s["tower_train"]))
    assert not bad, bad[:10]


def test_eval_loss_is_smaller_than_the_training_step(sizes):
    for c in CASES:
        for n in ROWS:
            s = sizes[case_id(c)][n]
            assert s["eval_loss"] < s["train_step"], (case_id(c), n, s)


def test_every_query_is_positive_and_grows_with_the_rows(sizes):
    for c in CASES:
        small, large = (sizes[case_id(c)][n] for n in ROWS)
        for q in QUERIES:
            assert 0 < small[q] < large[q], (case_id(c), q, small[q], large[q])


def test_sizes_match_the_library_before_the_shared_planner(sizes, parent):
    assert parent["queries"] == list(QUERIES) and parent["rows"] == list(ROWS)
    assert set(parent["sizes"]) == set(sizes)
    bad = []
    for cid, by_rows in sizes.items():
        for n in ROWS:
            old = dict(zip(QUERIES, parent["sizes"][cid][str(n)]))
            new = by_rows[n]
            for q in QUERIES[:4]:  # same buffers, every take 256-aligned: only the unpadded tail moves
                if abs(new[q] - old[q]) >= UNIT:
                    bad.append((cid, n, q, old[q], new[q]))
            # the old hand-written list over-took; the planner's size may only shrink
            if new["tower_forward"] > old["tower_forward"] + UNIT:
                bad.append((cid, n, "tower_forward", old["tower_forward"], new["tower_forward"]))
    assert not bad, bad[:10]
