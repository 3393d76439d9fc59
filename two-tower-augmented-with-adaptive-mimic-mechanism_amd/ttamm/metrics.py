"""Ranking metrics on the MI355X — drop-in for ``src/evaluation/metrics.py`` (:11-116) and for the
evaluation + metrics pair of the epoch loop (training.py:1522-1538, :1567-1583).

``ttamm_ranking_metrics`` (csrc/metrics.hip) computes Recall / Precision / NDCG / HitRate / MAP @K
and MRR of every query in one launch, a wave per query, and the means over the counted queries
in a fixed order.  Three ways in:

  * ``compute_ranking_metrics(per_user_predictions, per_user_ground_truth, k_values)`` — the
    reference's signature on dicts, packed with numpy;
  * ``ranking_metrics(pred_ids, truth_offsets, truth_values, k_values)`` — device tensors in;
  * ``evaluate_metrics(model, ...)`` — ``evaluate_model``'s arguments, the top-k ids go from the
    retrieval kernel to the metrics kernel without leaving HBM and no per-user dict is built.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Any, Iterable, Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .retrieval import _exact_operands, _group_pairs, _sampled_topk, blocked_csr, retrieve_topk
from .samplers import PositivesCSR

MAX_K = 192  # ttamm.h: a k and k_pred limit of ttamm_ranking_metrics
_NAMES = ("recall", "precision", "ndcg", "hit_rate", "map")


@dataclass(frozen=True)
class RankingMetrics:
    """metrics.py:11-19."""

    recall: dict[int, float]
    precision: dict[int, float]
    ndcg: dict[int, float]
    hit_rate: dict[int, float]
    map: dict[int, float]
    mrr: float
    per_user: list[dict[str, float]] = field(default_factory=list)


def _k_list(k_values: Iterable[int]) -> list[int]:
    ks = list(dict.fromkeys(int(k) for k in k_values))
    if not ks:
        raise ValueError("ttamm ranking metrics: k_values must not be empty")
    return ks


def _zeros(ks: Sequence[int]) -> RankingMetrics:
    """What the reference returns when no user is counted (_aggregate of an empty list, :101-105)."""
    return RankingMetrics(**{name: {k: 0.0 for k in ks} for name in _NAMES}, mrr=0.0, per_user=[])


def _result(ks: Sequence[int], summary: Sequence[float], rows: np.ndarray | None) -> RankingMetrics:
    out = {name: {k: float(summary[5 * j + m]) for j, k in enumerate(ks)} for m, name in enumerate(_NAMES)}
    per_user: list[dict[str, float]] = []
    if rows is not None:
        keys = [f"{name}@{k}" for k in ks for name in _NAMES] + ["mrr"]
        per_user = [dict(zip(keys, row)) for row in rows.tolist()]
    return RankingMetrics(**out, mrr=float(summary[5 * len(ks)]), per_user=per_user)


def _launch(pred_ids: torch.Tensor, truth_offsets: torch.Tensor, truth_values: torch.Tensor, ks: Sequence[int], *,
            pad_with_truth: bool, per_user: bool, extra: int = 0) -> tuple[torch.Tensor, torch.Tensor | None]:
    """One ttamm_ranking_metrics call: (summary [5 n_k + 2 + extra] on the device, per-user rows)."""
    dev = pred_ids.device
    nq, k_pred = pred_ids.shape
    ncol = 5 * len(ks) + 1
    lib = _lib.load()
    summary = torch.zeros(ncol + 1 + extra, dtype=torch.float64, device=dev)
    rows = torch.empty((nq, ncol), dtype=torch.float64, device=dev) if per_user else None
    ws_bytes = int(lib.ttamm_ranking_metrics_workspace_size(nq, len(ks)))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_ranking_metrics(
        pred_ids.data_ptr() if pred_ids.numel() else None, nq, k_pred, pred_ids.stride(0) if nq else k_pred,
        truth_offsets.data_ptr(), truth_values.data_ptr() if truth_values.numel() else None,
        (ctypes.c_int32 * len(ks))(*ks), len(ks), 1 if pad_with_truth else 0,
        rows.data_ptr() if rows is not None and nq else None, ncol, summary.data_ptr(), ws.data_ptr(), ws_bytes,
        _lib.stream_handle(dev)))
    return summary, rows


def ranking_metrics(pred_ids: torch.Tensor, truth_offsets: torch.Tensor, truth_values: torch.Tensor,
                    k_values: Iterable[int], *, pad_with_truth: bool = False, per_user: bool = False) -> RankingMetrics:
    """Metrics of ``pred_ids`` [n_queries, k_pred <= 192] (int64 ids, best first, ids < 0 =
    nothing there) against the truth CSR ``truth_values[truth_offsets[q]:truth_offsets[q + 1]]``
    (sorted ascending and unique per query).  Queries with no truth are not counted; with
    ``per_user`` the rows come back as the reference's list of dicts, one per COUNTED query in
    order.  ``pad_with_truth``: a list shorter than max(k_values) is followed by the query's
    unlisted truth items (training.py:969-972).  One host synchronisation: the summary read."""
    _lib.require_rocm(pred_ids, "ranking_metrics")
    ks = _k_list(k_values)
    dev = pred_ids.device
    if pred_ids.dtype != torch.long or pred_ids.dim() != 2 or (pred_ids.numel() and pred_ids.stride(1) != 1):
        raise ValueError("ttamm ranking_metrics: an int64 [n_queries, k_pred] id matrix with unit column stride is required")
    nq = pred_ids.shape[0]
    if pred_ids.shape[1] > MAX_K:  # nothing past max(k_values) <= 192 is ever read
        pred_ids = pred_ids[:, :MAX_K]
    if truth_offsets.dtype != torch.long or truth_values.dtype != torch.long or truth_offsets.numel() != nq + 1:
        raise ValueError("ttamm ranking_metrics: int64 truth_offsets [n_queries + 1] and truth_values are required")
    offsets = truth_offsets.to(dev).contiguous()
    values = truth_values.to(dev).contiguous()
    # the kernel trusts the offsets: hand it a copy that cannot leave truth_values, and report a
    # malformed CSR with the summary (same read)
    safe = offsets.clamp(0, values.numel())
    ok = (safe == offsets).all() & (safe[1:] >= safe[:-1]).all()
    summary, rows = _launch(pred_ids, safe, values, ks, pad_with_truth=pad_with_truth, per_user=per_user, extra=1)
    summary[-1] = ok.to(torch.float64)
    host = summary.cpu().tolist()
    if host[-1] != 1.0:
        raise ValueError("ttamm ranking_metrics: truth_offsets must be non-decreasing and lie inside truth_values")
    counted_rows = None
    if rows is not None:
        counted_rows = rows[(safe[1:] > safe[:-1])].cpu().numpy()
    return _result(ks, host, counted_rows)


def compute_ranking_metrics(per_user_predictions: Mapping[int, Sequence[int]],
                            per_user_ground_truth: Mapping[int, set[int]], k_values: Iterable[int], *,
                            device: torch.device | str | None = None, per_user: bool = True) -> RankingMetrics:
    """compute_ranking_metrics (metrics.py:74-116) in one kernel call: users in the predictions'
    order, users without ground truth skipped, ``per_user`` the list of ``{"recall@k": ...,
    "mrr": ...}`` dicts in that order.  Empty inputs return all-zero metrics without any device
    use (training.py:1679, :1683 call it with ``{}, {}``)."""
    ks = _k_list(k_values)
    max_k = max(ks)
    users = [u for u in per_user_predictions if per_user_ground_truth.get(u)]
    if not users:
        return _zeros(ks)
    if min(ks) < 1 or max_k > MAX_K:
        raise ValueError("ranking_metrics: every k must be in [1, 192]")
    preds = [np.asarray(per_user_predictions[u][:max_k], dtype=np.int64).reshape(-1) for u in users]
    truths = [np.fromiter(per_user_ground_truth[u], dtype=np.int64) for u in users]
    lens = np.fromiter((p.size for p in preds), dtype=np.int64, count=len(preds))
    flat = np.concatenate(preds) if preds else np.zeros(0, dtype=np.int64)
    tlens = np.fromiter((t.size for t in truths), dtype=np.int64, count=len(truths))
    tflat = np.concatenate(truths)
    if (flat.size and flat.min() < 0) or tflat.min() < 0:
        # the kernel reads ids < 0 as holes; the reference compares any integers: rank them
        _, inv = np.unique(np.concatenate([flat, tflat]), return_inverse=True)
        flat, tflat = inv[: flat.size].astype(np.int64), inv[flat.size:].astype(np.int64)
    k_pred = int(lens.max()) if lens.size else 0
    mat = np.full((len(users), max(k_pred, 1)), -1, dtype=np.int64)
    mat[np.arange(mat.shape[1])[None, :] < lens[:, None]] = flat
    toff = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(tlens, out=toff[1:])
    seg = np.repeat(np.arange(len(users), dtype=np.int64), tlens)
    tflat = tflat[np.lexsort((tflat, seg))]  # ascending within each user's segment
    dev = torch.device(device) if device is not None else torch.device("cuda")
    summary, rows = _launch(torch.from_numpy(mat).to(dev), torch.from_numpy(toff).to(dev),
                            torch.from_numpy(tflat).to(dev), ks, pad_with_truth=False, per_user=per_user)
    return _result(ks, summary.cpu().tolist(), rows.cpu().numpy() if rows is not None else None)


# ---------------------------------------------------------------------------------------
# evaluate_model + compute_ranking_metrics in one pass
# ---------------------------------------------------------------------------------------
def _pairs_tensor(val_interactions: Any, device: torch.device) -> torch.Tensor:
    """[n, 2] int64 (user, item) pairs on the device from a DataFrame (user_idx / item_idx
    columns, training.py:999), an iterable of pairs, or a tensor."""
    if isinstance(val_interactions, torch.Tensor):
        pairs = val_interactions
    elif hasattr(val_interactions, "groupby"):
        pairs = torch.from_numpy(np.ascontiguousarray(
            val_interactions[["user_idx", "item_idx"]].to_numpy(dtype=np.int64)))
    else:
        pairs = torch.from_numpy(np.asarray(val_interactions, dtype=np.int64).reshape(-1, 2))
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("ttamm evaluate_metrics: val_interactions must be [n, 2] (user, item) pairs")
    return pairs.to(device=device, dtype=torch.long)


def truth_csr(pairs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(users, offsets, values) of [n, 2] (user, item) pairs with tensor ops: users ascending (as
    DataFrame.groupby yields them, training.py:999), each user's items ascending and unique."""
    uniq = torch.unique(pairs, dim=0)  # rows in lexicographic order
    users, counts = torch.unique_consecutive(uniq[:, 0], return_counts=True)
    offsets = torch.zeros(users.numel() + 1, dtype=torch.long, device=pairs.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    return users, offsets, uniq[:, 1].contiguous()


def select_blocked_csr(csr: PositivesCSR, users: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The rows ``users`` of a device PositivesCSR as the blocked CSR of retrieve_topk, with
    tensor ops (a user outside the CSR has no positives, as ``positives.get(u, ())``)."""
    dev = users.device
    n = users.numel()
    if csr.num_users == 0 or n == 0:
        return torch.zeros(n + 1, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev)
    off = csr.offsets.to(dev)
    inside = (users >= 0) & (users < csr.num_users)
    row = users.clamp(0, csr.num_users - 1)
    start = off[row]
    length = torch.where(inside, off[row + 1] - start, torch.zeros_like(start))
    boff = torch.zeros(n + 1, dtype=torch.long, device=dev)
    torch.cumsum(length, 0, out=boff[1:])
    total = int(boff[-1])
    query = torch.repeat_interleave(torch.arange(n, device=dev), length, output_size=total)
    src = torch.arange(total, device=dev) - boff[query] + start[query]
    return boff, csr.values.to(dev)[src]


class _CSRMapping:
    """``blocked.get(u, ())`` over a PositivesCSR's host copy (the sampled branch draws on the host)."""

    def __init__(self, csr: PositivesCSR) -> None:
        self.offsets = csr.offsets.cpu().numpy()
        self.values = csr.values.cpu().numpy()

    def get(self, u: int, default: Any = ()) -> Any:
        if 0 <= u < self.offsets.size - 1:
            return self.values[self.offsets[u]:self.offsets[u + 1]].tolist()
        return default


def evaluate_metrics(
    model,
    *,
    train_positive_map: Mapping[int, set[int]] | PositivesCSR,
    val_interactions: Any,
    item_feature_tensor: torch.Tensor | None,
    user_feature_tensor: torch.Tensor | None,
    device: torch.device,
    num_items: int,
    candidate_samples: int = 0,
    k_values: Iterable[int] = (20,),
    rng: Any = None,
    faiss_resources: Any = None,
    faiss_search_k: int = 0,
    item_embeddings: torch.Tensor | None = None,
    per_user: bool = False,
) -> RankingMetrics:
    """``compute_ranking_metrics(*evaluate_model(...), k_values)`` (training.py:1522-1538) without
    the per-user dicts: ``evaluate_model``'s arguments and branch rules; ``val_interactions`` may
    also be a [n, 2] int64 tensor and ``train_positive_map`` a device PositivesCSR (the
    sampler's).  The truth CSR is built with tensor ops; in the exact branches the top-k ids go
    straight from ``ttamm_retrieval_topk`` into ``ttamm_ranking_metrics`` (pad_with_truth), and
    with tensor / PositivesCSR inputs nothing loops over users or pairs on the host.  The
    sampled-candidate branch draws its candidates on the host in the reference's order
    (``sampled_candidates``) and maps the ranked list positions to ids with a device gather."""
    ks = _k_list(k_values)
    max_k = max(ks)
    device = torch.device(device)
    sampled = faiss_resources is None and rng is not None and item_embeddings is None
    if not isinstance(val_interactions, torch.Tensor) and not hasattr(val_interactions, "groupby"):
        val_interactions = list(val_interactions)  # read once (it may be a generator)
    pairs = _pairs_tensor(val_interactions, device)
    if pairs.shape[0] == 0:
        return _zeros(ks)
    model.eval()
    users, toff, tval = truth_csr(pairs)
    if sampled:
        # the candidate lists' order is that of the reference's sets, built in the pairs' order
        host_pairs = val_interactions if not isinstance(val_interactions, torch.Tensor) else pairs.cpu().tolist()
        groups = _group_pairs(host_pairs)
        user_list = [u for u, items in groups.items() if items]
        truth = {u: set(groups[u]) for u in user_list}
        blocked = _CSRMapping(train_positive_map) if isinstance(train_positive_map, PositivesCSR) else train_positive_map
        _, flat, offsets, pos = _sampled_topk(model, user_list, truth, blocked, item_features=item_feature_tensor,
                                              user_features=user_feature_tensor, device=device, num_items=num_items,
                                              candidate_samples=candidate_samples, max_k=max_k, rng=rng)
        flat_d = torch.from_numpy(flat).to(device)
        off_d = torch.from_numpy(offsets).to(device)
        length = (off_d[1:] - off_d[:-1]).unsqueeze(1)
        inside = (pos >= 0) & (pos < length)  # positions past a short list are holes
        src = (off_d[:-1].unsqueeze(1) + pos.clamp(min=0)).clamp(max=max(flat.size - 1, 0))
        ids = torch.where(inside, flat_d[src] if flat.size else torch.full_like(pos, -1), torch.full_like(pos, -1))
        return ranking_metrics(ids, toff, tval, ks, pad_with_truth=False, per_user=per_user)
    q, items = _exact_operands(model, users, faiss_resources=faiss_resources, item_embeddings=item_embeddings,
                               item_feature_tensor=item_feature_tensor, user_feature_tensor=user_feature_tensor,
                               device=device, num_items=num_items)
    if isinstance(train_positive_map, PositivesCSR):
        boff, bval = select_blocked_csr(train_positive_map, users)
    else:
        boff, bval = blocked_csr(users.tolist(), train_positive_map, device)
    _, ids = retrieve_topk(q, items, max_k, blocked_offsets=boff, blocked_values=bval)
    return ranking_metrics(ids, toff, tval, ks, pad_with_truth=True, per_user=per_user)
