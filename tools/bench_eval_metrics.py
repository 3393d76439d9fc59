#!/usr/bin/env python3
"""Evaluation + ranking metrics at BASELINE config C3's retrieval shape (65,536 queries x 2M items x
96, k_values = [5, 10, 20], 20 blocked items and 1-5 truth items per query; synthetic embeddings,
no model): what follows the top-k kernel, two ways, alternating in one process after a warm-up
of both:

  (a) host:   the path before ttamm.ranking_metrics existed — `retrieve_topk` -> `ids.cpu().tolist()`
              -> per-user lists (filter, pad with the truth, cut: ttamm/retrieval.py `_exact`) ->
              the per-user metric loop (oracle.cpu_reference.ranking_metrics, the restatement of
              src/evaluation/metrics.py:74-116);
  (b) device: the same `retrieve_topk`, then `ttamm.ranking_metrics` on the ids where they are
              (one kernel call, one summary read).

    python tools/bench_eval_metrics.py [--config c3] [--rounds 5] [--out profiles/eval_metrics_c3.json]

Each round times the retrieval (device events, synchronised) and then the post-retrieval part
(host clock; both variants end in a device-to-host read, so the clock stops after the device is
done).  Prints one JSON line (and writes it to --out): medians with min / max, the end-to-end
ratio (retrieval + post, (a) over (b)), the metrics launch's device time and its bytes from
shapes.  (b) does strictly less on the host, so the exit status is 1 when its post-retrieval time
is not below (a)'s, or when the two disagree by more than 1e-12."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"))

import torch  # noqa: E402

CONFIGS = {
    "c3": dict(nq=65_536, ni=2_000_000, D=96, blocked=20),
    "tiny": dict(nq=1_000, ni=5_000, D=32, blocked=20),
}
KS = [5, 10, 20]
NAMES = ("recall", "precision", "ndcg", "hit_rate", "map")


def host_post(ids: torch.Tensor, users: range, truth: dict, max_k: int):
    """What evaluate_model + compute_ranking_metrics did after the kernel (retrieval.py `_exact`)."""
    from oracle import cpu_reference as ref

    preds = {}
    for u, row in zip(users, ids.cpu().tolist()):
        got = [i for i in row if i >= 0]
        if len(got) < max_k:
            seen = set(got)
            got.extend(i for i in truth[u] if i not in seen)
        preds[u] = got[:max_k]
    return ref.ranking_metrics(preds, truth, KS)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics needs the MI355X (no CPU fallback)")
    import ttamm
    from ttamm.retrieval import retrieve_topk

    c = CONFIGS[args.config]
    nq, ni, D, nb = c["nq"], c["ni"], c["D"], c["blocked"]
    max_k = max(KS)
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    items = torch.randn((ni, D), device=dev)
    queries = torch.randn((nq, D), device=dev)
    boff = torch.arange(0, nb * nq + 1, nb, device=dev)
    bval = torch.randint(0, ni, (nq, nb), device=dev).sort(dim=1).values.reshape(-1)
    # truth: 1-5 items per query, the first three taken from the query's real top-20 so that hits occur
    _, top = retrieve_topk(queries, items, max_k, blocked_offsets=boff, blocked_values=bval)
    g = torch.Generator().manual_seed(args.seed + 1)
    n_truth = torch.randint(1, 6, (nq,), generator=g)
    where = torch.rand((nq, max_k), generator=g).argsort(dim=1)[:, :3]  # three list positions per query
    cand = torch.cat([top.cpu().gather(1, where), torch.randint(0, ni, (nq, 2), generator=g)], dim=1)
    truth = {q: set(row[:n]) for q, (row, n) in enumerate(zip(cand.tolist(), n_truth.tolist()))}
    sizes = torch.tensor([len(truth[q]) for q in range(nq)])
    toff = torch.zeros(nq + 1, dtype=torch.long)
    toff[1:] = sizes.cumsum(0)
    tval = torch.tensor([i for q in range(nq) for i in sorted(truth[q])], dtype=torch.long)
    toff, tval = toff.to(dev), tval.to(dev)
    users = range(nq)

    def retrieval():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _, ids = retrieve_topk(queries, items, max_k, blocked_offsets=boff, blocked_values=bval)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), ids

    def post_host(ids):
        return host_post(ids, users, truth, max_k)

    def post_device(ids):
        return ttamm.ranking_metrics(ids, toff, tval, KS, pad_with_truth=True)

    variants = {"host": post_host, "device": post_device}
    for fn in variants.values():  # every code object and shape of the timed windows
        fn(retrieval()[1])
    retr = []
    post = {k: [] for k in variants}
    total = {k: [] for k in variants}
    result = {}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            ms, ids = retrieval()
            t0 = time.perf_counter()
            result[name] = fn(ids)
            p = (time.perf_counter() - t0) * 1e3
            retr.append(ms)
            post[name].append(p)
            total[name].append(ms + p)
    # the metrics launch alone (kernel + fixed-order reduction), device events
    _, ids = retrieval()
    lib_ms = []
    from ttamm.metrics import _launch
    for _ in range(args.rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _launch(ids, toff, tval, KS, pad_with_truth=True, per_user=False)
        b.record()
        torch.cuda.synchronize()
        lib_ms.append(a.elapsed_time(b))
    lib_ms = lib_ms[1:]

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    diff = max(max(abs(getattr(result["host"], n)[k] - getattr(result["device"], n)[k]) for n in NAMES for k in KS),
               abs(result["host"].mrr - result["device"].mrr))
    med_post = {k: statistics.median(v) for k, v in post.items()}
    med_total = {k: statistics.median(v) for k, v in total.items()}
    chunks = (nq + 255) // 256
    kernel_bytes = 8 * (nq * max_k + (nq + 1) + int(tval.numel()) + chunks * 42 + 5 * len(KS) + 2)
    ok_time, ok_same = med_post["device"] < med_post["host"], diff <= 1e-12
    line = {
        "metric": "evaluation after the top-k kernel: retrieval (device events) + post-retrieval (host clock, ends in a device-to-host read), ms",
        "config": {"name": args.config, "queries": nq, "items": ni, "dim": D, "k_values": KS, "blocked_per_query": nb,
                   "truth_per_query": "1-5", "truth_items": int(tval.numel())},
        "rounds": args.rounds,
        "retrieval_ms": stat(retr),
        "post_retrieval_ms": {k: stat(v) for k, v in post.items()},
        "end_to_end_ms": {k: stat(v) for k, v in total.items()},
        "end_to_end_host_over_device": round(med_total["host"] / med_total["device"], 2),
        "post_retrieval_host_over_device": round(med_post["host"] / med_post["device"], 1),
        "metrics_launch_device_ms": stat(lib_ms),
        "metrics_kernel_bytes": kernel_bytes,
        "metrics_kernel_GBps": round(kernel_bytes / (statistics.median(lib_ms) * 1e-3) / 1e9, 2),
        "recall": {str(k): result["device"].recall[k] for k in KS},
        "ndcg": {str(k): result["device"].ndcg[k] for k in KS},
        "mrr": result["device"].mrr,
        "max_abs_diff_host_vs_device": diff,
        "conditions": {"device_post_below_host_post": ok_time, "same_within_1e-12": ok_same},
    }
    text = json.dumps(line)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    return 0 if ok_time and ok_same else 1


if __name__ == "__main__":
    sys.exit(main())
