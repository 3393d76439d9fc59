"""Row-sharded evaluation: exact top-k retrieval and ranking metrics over W ranks.

The model of ``ttamm.sharded`` keeps item i on rank i % W at local row i // W, and each rank's
queries are its own users.  Nothing here gathers a table: per round of at most ``query_block``
queries per rank

  all-gather   the ranks' query blocks, padded to qb rows           [W qb, D] fp32 per rank
  a2a          (local item row, query slot) of every blocked pair -> the item's owner
  scan         ttamm_retrieval_topk of all W qb queries over the rank's item shard
  a2a          the partial lists back to the queries' owners: scores [W qb, k] fp32 and local
               rows [W qb, k] int64, two exchanges of one layout (ttamm_topk_merge reads both
               through one pair of element strides, so they are not packed into one buffer)
  merge        ttamm_topk_merge with id_stride = W: local row * W + source rank is the item id

so the result is ``retrieve_topk`` over the global item matrix, tie order included.  The
programs yield the collective requests of ``ttamm.sharded`` (TorchComm, MirrorComm and
run_loopback serve them).
"""

from __future__ import annotations

import dataclasses
import functools
from typing import Any, Callable, Iterable, Mapping

import torch

from . import _lib
from .metrics import (_NAMES, MAX_K, RankingMetrics, _k_list, _pairs_tensor, _result, _zeros, ranking_metrics,
                      select_blocked_csr, truth_csr)
from .retrieval import (_uses_cosine, blocked_csr, encode_item_embeddings, encode_user_embeddings, normalize_rows,
                        retrieve_topk, topk_merge)
from .samplers import PositivesCSR
from .sharded import AllGather, AllReduce, AllToAll, Program, Router, RowOwnership, device_route


def _mark(timeline: list | None, name: str) -> None:
    """Stage boundary for tools/bench_eval_sharded.py: a device event after the stage ``name``."""
    if timeline is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        timeline.append((name, ev))


def route_blocked(own: RowOwnership, router: Router, blocked_offsets: torch.Tensor, blocked_values: torch.Tensor,
                  query_base: int, n_slots: int) -> Program:
    """Program: this rank's block of queries — blocked CSR ``blocked_offsets`` [n + 1] over
    ``blocked_values`` (GLOBAL item ids, ascending per query), query j being slot
    ``query_base + j`` of the round's ``n_slots`` = W qb slots — to the owner-side CSR.  Returns
    (offsets [n_slots + 1], values): per slot the LOCAL rows (i // W) of its blocked items that
    this rank owns, ascending.

    Each (slot, item) pair goes to rank item % W through the router, the slot as payload.  The
    router is stable, sources arrive in rank order and slots are rank-major, so the received pairs
    are already sorted by (slot, item): the offsets are a count per slot.  The W x W count matrix
    is all-gathered once (one host sync) and gives the splits, as in ``route_pairs``."""
    W = own.world_size
    off = blocked_offsets.reshape(-1)
    n = off.numel() - 1
    dev = off.device
    lens = off[1:] - off[:-1]
    lo, hi = (int(off[0]), int(off[-1])) if n > 0 else (0, 0)
    values = blocked_values.reshape(-1)[lo:hi]
    slots = torch.repeat_interleave(torch.arange(query_base, query_base + n, dtype=torch.long, device=dev), lens,
                                    output_size=hi - lo)
    packed, _, counts = router(W, values, None, slots)
    if W > 1:
        m = yield AllGather(counts)
        m = m.reshape(W, W).tolist()  # m[src][dst]
        packed = yield AllToAll(packed, m[own.rank], [m[src][own.rank] for src in range(W)])
    per_slot = torch.bincount(packed[:, 1], minlength=n_slots)
    offsets = torch.zeros(n_slots + 1, dtype=torch.long, device=dev)
    torch.cumsum(per_slot, 0, out=offsets[1:])
    return offsets, packed[:, 0].contiguous()


def _default_router() -> Router:
    return functools.partial(device_route, _lib.load())


def retrieve_topk_program(own: RowOwnership, queries: torch.Tensor, items_local: torch.Tensor, k: int, *,
                          blocked_offsets: torch.Tensor | None = None, blocked_values: torch.Tensor | None = None,
                          router: Router | None = None, query_block: int = 65536,
                          timeline: list | None = None) -> Program:
    """Program: ``retrieve_topk`` of this rank's ``queries`` [nq, D] over the GLOBAL item matrix
    whose rows i % W == rank are ``items_local`` (row i // W).  ``blocked_offsets`` /
    ``blocked_values``: this rank's queries' blocked GLOBAL item ids (CSR, ascending per query).
    Returns (scores [nq, k], ids [nq, k]) with global item ids, ordered as ``retrieve_topk``
    orders them (score descending, then item id).

    Collective: every rank calls it, with any number of queries (zero included).  One all-gather
    of (query count, blocked count) fixes the rounds and the padded block size qb <=
    ``query_block``; a round moves W qb D 4 bytes of queries in and W qb k 12 bytes of partial
    lists out per rank, and each blocked pair once.  World size 1 issues no collective."""
    if (blocked_offsets is None) != (blocked_values is None):
        raise ValueError("ttamm retrieval: blocked_offsets and blocked_values go together")
    if query_block < 1:
        raise ValueError("ttamm retrieval: query_block must be >= 1")
    W, rank = own.world_size, own.rank
    if W == 1:
        return retrieve_topk(queries, items_local, k, blocked_offsets=blocked_offsets, blocked_values=blocked_values)
    _lib.require_rocm(queries, "retrieve_topk_program")
    nq, D = queries.shape
    dev = queries.device
    if blocked_offsets is not None and blocked_offsets.numel() != nq + 1:
        raise ValueError("ttamm retrieval: blocked_offsets must have n_queries + 1 entries")
    router = router or _default_router()
    n_blocked = int(blocked_values.numel()) if blocked_values is not None else 0
    sizes = yield AllGather(torch.tensor([[nq, n_blocked]], dtype=torch.long, device=dev))
    sizes = sizes.tolist()
    most = max(s[0] for s in sizes)
    any_blocked = any(s[1] for s in sizes)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, k), dtype=torch.long, device=dev)
    if most == 0:
        return out_s, out_i
    rounds = (most + query_block - 1) // query_block
    qb = (most + rounds - 1) // rounds
    if any_blocked and blocked_offsets is None:
        blocked_offsets = torch.zeros(nq + 1, dtype=torch.long, device=dev)
        blocked_values = torch.zeros(0, dtype=torch.long, device=dev)
    for r in range(rounds):
        lo = min(nq, r * qb)
        hi = min(nq, lo + qb)
        n = hi - lo
        _mark(timeline, "start")
        block = torch.zeros((qb, D), dtype=torch.float32, device=dev)  # padded rows: zero queries, dropped below
        block[:n] = queries[lo:hi]
        everyone = yield AllGather(block)
        _mark(timeline, "gather")
        ooff = oval = None
        if any_blocked:
            ooff, oval = yield from route_blocked(own, router, blocked_offsets[lo:hi + 1], blocked_values, rank * qb,
                                                  W * qb)
        _mark(timeline, "route_blocked")
        part_s, part_i = retrieve_topk(everyone, items_local, k, blocked_offsets=ooff, blocked_values=oval)
        _mark(timeline, "scan")
        # rows [d qb, (d + 1) qb) are rank d's queries: back to it; what arrives is list-major [W, qb, k]
        got_s = yield AllToAll(part_s, [qb] * W, [qb] * W)
        got_i = yield AllToAll(part_i, [qb] * W, [qb] * W)
        _mark(timeline, "return")
        ms, mi = topk_merge(got_s.view(W, qb, k), got_i.view(W, qb, k), k, id_stride=W)
        out_s[lo:hi] = ms[:n]
        out_i[lo:hi] = mi[:n]
        _mark(timeline, "merge")
    return out_s, out_i


def evaluate_metrics_program(
    model,
    own: RowOwnership,
    *,
    train_positive_map: Mapping[int, Iterable[int]] | PositivesCSR,
    val_interactions: Any,
    item_feature_tensor: torch.Tensor | None,
    user_feature_tensor: torch.Tensor | None,
    num_items: int,
    k_values: Iterable[int] = (20,),
    item_embeddings: torch.Tensor | None = None,
    per_user: bool = False,
    router: Router | None = None,
    query_block: int = 65536,
    candidate_samples: int = 0,
    rng: Any = None,
) -> Program:
    """``ttamm.evaluate_metrics`` (exact search) for one rank of a row-sharded model, as a program.

    ``model`` is the rank's shard (``ShardedTrainStep``'s conventions throughout): the feature
    tensors are the rank's rows, ``train_positive_map`` (a PositivesCSR or a mapping) is keyed
    by LOCAL user row and holds GLOBAL item ids, ``num_items`` is the global item count, and
    ``val_interactions`` is [n, 2] (LOCAL user row, GLOBAL item id) of users this rank owns.
    Pairs of arbitrary users go through ``route_pairs`` first::

        u, i, _ = yield from route_pairs(own, router, global_users, items)
        metrics = yield from evaluate_metrics_program(model, own, val_interactions=torch.stack([u, i], 1), ...)

    The rank encodes its item shard and its queries (L2-normalised for a cosine model), runs
    ``retrieve_topk_program`` for max(k_values), ``ranking_metrics(pad_with_truth=True)`` on its own
    queries, and one fp64 all-reduce of (mean x count per column, count) gives every rank the same
    global means.  ``per_user=True``: the rows of THIS rank's users, in its order.  ``item_embeddings``
    may be the rank's already encoded shard.  Without a validation pair on any rank the result is
    the all-zero RankingMetrics, reached after the same collectives on every rank.  The
    sampled-candidate branch (``rng`` / ``candidate_samples``) is not sharded: NotImplementedError,
    raised here, before any collective."""
    if rng is not None or candidate_samples:
        raise NotImplementedError("ttamm: the sampled-candidate evaluation (rng= / candidate_samples) is not sharded; "
                                  "use the exact search")
    ks = _k_list(k_values)
    if min(ks) < 1 or max(ks) > MAX_K:
        raise ValueError("ranking_metrics: every k must be in [1, 192]")
    return _evaluate_metrics(model, own, ks, train_positive_map, val_interactions, item_feature_tensor,
                             user_feature_tensor, int(num_items), item_embeddings, per_user, router, query_block)


def _evaluate_metrics(model, own, ks, train_positive_map, val_interactions, item_feature_tensor, user_feature_tensor,
                      num_items, item_embeddings, per_user, router, query_block) -> Program:
    max_k = max(ks)
    device = next(model.parameters()).device
    if not isinstance(val_interactions, torch.Tensor) and not hasattr(val_interactions, "groupby"):
        val_interactions = list(val_interactions)
    pairs = _pairs_tensor(val_interactions, device)
    model.eval()
    if item_embeddings is None:
        items = encode_item_embeddings(model, num_items=own.local_count(num_items), item_features=item_feature_tensor,
                                       device=device)
    else:
        items = item_embeddings.clone() if _uses_cosine(model) else item_embeddings
    if pairs.shape[0]:
        users, toff, tval = truth_csr(pairs)
    else:
        users = torch.zeros(0, dtype=torch.long, device=device)
        toff = torch.zeros(1, dtype=torch.long, device=device)
        tval = torch.zeros(0, dtype=torch.long, device=device)
    q = encode_user_embeddings(model, users, user_features=user_feature_tensor)
    if q.shape[1] != items.shape[1]:  # a rank without queries: the empty matrix takes the items' width
        q = q.new_empty((q.shape[0], items.shape[1]))
    if _uses_cosine(model):  # normalize_L2 on the index and on every query (training.py:670-672, :954-955)
        normalize_rows(items)
        normalize_rows(q)
    if isinstance(train_positive_map, PositivesCSR):
        boff, bval = select_blocked_csr(train_positive_map, users)
    else:
        boff, bval = blocked_csr(users.tolist(), train_positive_map, device)
    _, ids = yield from retrieve_topk_program(own, q, items, max_k, blocked_offsets=boff, blocked_values=bval,
                                              router=router, query_block=query_block)
    ncol = 5 * len(ks) + 1
    share = [0.0] * (ncol + 1)  # this rank's column sums (mean x count), then its count
    local = None
    if users.numel():
        local = ranking_metrics(ids, toff, tval, ks, pad_with_truth=True, per_user=per_user)
        # every user of truth_csr has a truth item, so every local query is counted
        count = float(users.numel())
        means = [getattr(local, name)[k] for k in ks for name in _NAMES] + [local.mrr]
        share = [m * count for m in means] + [count]
    if own.world_size == 1:  # the one-process evaluate_metrics, bit for bit
        return local if local is not None else _zeros(ks)
    share = torch.tensor(share, dtype=torch.float64).to(device)
    yield AllReduce(share)
    total = share.cpu().tolist()
    if total[ncol] == 0:
        return _zeros(ks)
    out = _result(ks, [v / total[ncol] for v in total[:ncol]], None)
    return dataclasses.replace(out, per_user=local.per_user if local is not None else [])


def evaluate_metrics_sharded(model, own: RowOwnership, *, comm: Callable[[Program], Any], **kw: Any) -> RankingMetrics:
    """``evaluate_metrics_program`` run to completion by ``comm`` (e.g. ``TorchComm()``).  Collective:
    every rank calls it with its own shard, users and pairs (see ``evaluate_metrics_program``)."""
    if comm is None:
        raise RuntimeError("ttamm: evaluate_metrics_sharded needs comm= (e.g. TorchComm())")
    runner = comm.run if hasattr(comm, "run") else comm
    return runner(evaluate_metrics_program(model, own, **kw))
