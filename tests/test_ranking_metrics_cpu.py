"""ttamm_ranking_metrics / ttamm.compute_ranking_metrics: everything that is decided before any
device work (the library loads without a GPU, as tests/test_abi_cpu.py shows)."""

from __future__ import annotations

import ctypes
import dataclasses

import pytest

import ttamm
from ttamm import _lib

FAKE = 4096  # placeholder pointers, never dereferenced: validation fails first


def _call(**over):
    """A call that would be valid (3 queries, 20 ids each, k = 5, 10, 20, per-user rows) with
    ``over`` applied: each test breaks exactly one thing."""
    lib = _lib.load()
    a = dict(pred_ids=FAKE, n_queries=3, k_pred=20, ld_pred=20, truth_offsets=FAKE, truth_values=FAKE,
             k_values=[5, 10, 20], pad_with_truth=0, per_user=FAKE, ld_per_user=16, summary=FAKE, workspace=FAKE,
             workspace_bytes=None)
    a.update(over)
    ks = a["k_values"]
    n_k = a.pop("n_k", len(ks))
    karr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.ttamm_ranking_metrics_workspace_size(a["n_queries"], max(1, min(n_k, 8)))
    return lib.ttamm_ranking_metrics(a["pred_ids"], a["n_queries"], a["k_pred"], a["ld_pred"], a["truth_offsets"],
                                     a["truth_values"], karr, n_k, a["pad_with_truth"], a["per_user"],
                                     a["ld_per_user"], a["summary"], a["workspace"], a["workspace_bytes"], None)


@pytest.mark.parametrize("over,match", [
    (dict(k_values=[], n_k=0), r"n_k must be in \[1, 8\]"),
    (dict(k_values=list(range(1, 10))), r"n_k must be in \[1, 8\]"),
    (dict(k_values=[5, 0, 20]), r"every k must be in \[1, 192\]"),
    (dict(k_values=[5, 193]), r"every k must be in \[1, 192\]"),
    (dict(k_pred=-1), r"k_pred must be in \[0, 192\]"),
    (dict(k_pred=193, ld_pred=193), r"k_pred must be in \[0, 192\]"),
    (dict(ld_pred=19), "ld_pred"),
    (dict(ld_per_user=15), "ld_per_user"),
    (dict(summary=None), "summary, truth_offsets and workspace"),
    (dict(truth_offsets=None), "summary, truth_offsets and workspace"),
    (dict(workspace=None), "summary, truth_offsets and workspace"),
    (dict(pred_ids=None), "null pred_ids"),
    (dict(workspace_bytes=8), "workspace too small"),
])
def test_invalid_arguments_are_rejected_before_any_device_work(over, match):
    with pytest.raises(ValueError, match=match):
        _lib.check(_call(**over))


def test_ld_per_user_is_only_checked_when_rows_are_asked_for():
    """ld_per_user < 5 n_k + 1 is fine without per_user: the next defect is the one reported."""
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(_call(per_user=None, ld_per_user=0, workspace_bytes=8))


def test_workspace_size_is_nonzero_and_grows_with_the_queries():
    lib = _lib.load()
    small = lib.ttamm_ranking_metrics_workspace_size(1, 3)
    assert small > 0
    assert lib.ttamm_ranking_metrics_workspace_size(0, 3) > 0  # the zero summary still wants a workspace
    assert lib.ttamm_ranking_metrics_workspace_size(70_000, 3) > small
    assert lib.ttamm_ranking_metrics_workspace_size(1_000_000, 3) > lib.ttamm_ranking_metrics_workspace_size(70_000, 3)


def test_empty_inputs_return_zeros_without_a_device():
    """training.py:1679, :1683 call compute_ranking_metrics({}, {}, ks)."""
    m = ttamm.compute_ranking_metrics({}, {}, [5, 10])
    for name in ("recall", "precision", "ndcg", "hit_rate", "map"):
        assert getattr(m, name) == {5: 0.0, 10: 0.0}
    assert m.mrr == 0.0 and m.per_user == []
    # users without ground truth are skipped, so this is empty too
    m = ttamm.compute_ranking_metrics({3: [1, 2]}, {3: set(), 4: {1}}, [5])
    assert m.recall == {5: 0.0} and m.per_user == []


def test_ranking_metrics_has_the_reference_fields():
    """metrics.py:11-19."""
    assert [f.name for f in dataclasses.fields(ttamm.RankingMetrics)] == [
        "recall", "precision", "ndcg", "hit_rate", "map", "mrr", "per_user"]
    assert ttamm.RankingMetrics.__dataclass_params__.frozen
    for name in ("RankingMetrics", "compute_ranking_metrics", "ranking_metrics", "evaluate_metrics"):
        assert name in ttamm.__all__
