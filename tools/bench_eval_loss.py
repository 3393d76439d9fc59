#!/usr/bin/env python3
"""Validation-loss pass at BASELINE config C2 (2M x 200K tables, F = 605 -> 192 -> 96, B = 8192,
N = 5): time per batch of three ways through the same K batches, alternating in one process,
device events around each window of K batches after a warm-up of every variant:

  (a) module:  the body of `_compute_loss` (training.py:854-910) as the reference runs it on the
               ttamm module classes — `ttamm.sample_negative_items`, `index_select` of the feature
               rows, three tower forwards, three augments, torch elementwise ops, `loss.item()`;
  (b) fused:   `ttamm.compute_loss` (one `ttamm_eval_loss` call per batch, one synchronise per pass);
               `engine_step` is the same pass on an engine built once (no per-pass set-up);
  (c) train:   `FusedTrainStep.step` on the same batches (the fused training step next to it).

    python tools/bench_eval_loss.py [--config c2] [--batches 100] [--rounds 5] [--out FILE]

Prints one JSON line (and writes it to --out): the median over the rounds of each variant's
ms/batch with its min / max, the (a)/(b) ratio, and the scorer's read bytes from shapes,
4 D B (2 + N).  The pass runs a strict subset of the step's kernels on the same rows, so (b) must
come out below (c), and below (a); the exit status is 1 when either fails."""

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
from torch import nn  # noqa: E402


def module_compute_loss(model, batches, *, criterion, negatives_per_positive, num_items, user_positive_items,
                        user_features, item_features, device) -> float:
    """`_compute_loss` (training.py:836-914) as written, on the swapped module classes."""
    import ttamm

    model.eval()
    running_loss, total_samples = 0.0, 0
    mimic = getattr(model, "adaptive_mimic", None)
    with torch.no_grad():
        for users, pos in batches:
            users, pos = users.to(device), pos.to(device)
            neg = ttamm.sample_negative_items(users, num_items=num_items, positives=user_positive_items,
                                              num_negatives=negatives_per_positive, device=device)
            u = model.user_encoder({"indices": users, "features": user_features.index_select(0, users)})
            p = model.item_encoder({"indices": pos, "features": item_features.index_select(0, pos)})
            if mimic is not None:
                u = mimic.augment_users(users, u)
                p = mimic.augment_items(pos, p)
            pos_logits = (u * p).sum(dim=-1)
            neg_flat = neg.view(-1)
            n = model.item_encoder({"indices": neg_flat, "features": item_features.index_select(0, neg_flat)})
            if mimic is not None:
                n = mimic.augment_items(neg_flat, n)
            n = n.view(-1, negatives_per_positive, u.shape[-1])
            neg_logits = (u.unsqueeze(1) * n).sum(dim=-1)
            logits = torch.cat([pos_logits, neg_logits.reshape(-1)], dim=0)
            labels = torch.cat([torch.ones_like(pos_logits), torch.zeros_like(neg_logits.reshape(-1))], dim=0)
            loss = criterion(logits, labels)
            running_loss += loss.item() * pos_logits.shape[0]
            total_samples += pos_logits.shape[0]
    return running_loss / total_samples if total_samples else 0.0


def timed(fn) -> tuple[float, float, object]:
    """(device ms, wall ms, result) of fn(), events on the current stream, synchronised."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "tiny"])
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_loss needs the MI355X (no CPU fallback)")
    import bench
    import ttamm

    c = bench.CONFIGS[args.config]
    dev = torch.device("cuda")
    w = bench.Workload(c, dev, args.seed)
    K = args.batches
    batches = [w.batch() for _ in range(K)]
    kw = dict(criterion=nn.BCEWithLogitsLoss(), negatives_per_positive=c["N"], num_items=c["I"],
              user_positive_items=w.csr, user_features=w.user_features, item_features=w.item_features, device=dev)
    engine = ttamm.FusedEvalLoss(w.model, negatives_per_positive=c["N"], positives=w.csr,
                                 user_features=w.user_features, item_features=w.item_features, max_batch=c["B"],
                                 seed=args.seed)

    def run_module(bs):
        return module_compute_loss(w.model, bs, **kw)

    def run_fused(bs):
        return ttamm.compute_loss(w.model, bs, seed=args.seed, **kw)

    def run_engine(bs):
        for u, p in bs:
            engine.step(u, p)
        return engine.finish()

    def run_train(bs):
        for u, p in bs:
            w.engine.step(u, p)
        return None

    variants = {"module": run_module, "fused": run_fused, "engine_step": run_engine, "train": run_train}
    for fn in variants.values():  # every shape and code object of the timed windows
        fn(batches[: args.warmup])
    w.engine.flush()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    losses = {}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            d, h, out = timed(lambda fn=fn: fn(batches))
            if name == "train":  # outside the window: the deferred tables brought current for the passes
                w.engine.flush()
            ms[name].append(d / K)
            wall[name].append(h / K)
            losses[name] = out
    w.engine.finish()

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    med = {k: statistics.median(v) for k, v in ms.items()}
    B, N, D = c["B"], c["N"], c["D"]
    ok_c, ok_a = med["fused"] < med["train"], med["fused"] < med["module"]
    line = {
        "metric": "validation-loss pass, ms per batch (device events around K batches)",
        "config": {"name": args.config, **{k: c[k] for k in ("U", "I", "F", "H", "D", "B", "N")}},
        "batches": K, "rounds": args.rounds, "warmup_batches": args.warmup,
        "ms_per_batch": {k: stat(v) for k, v in ms.items()},
        "wall_ms_per_batch": {k: stat(v) for k, v in wall.items()},
        "module_over_fused": round(med["module"] / med["fused"], 2),
        "fused_over_train": round(med["fused"] / med["train"], 3),
        "interactions_per_s_fused": round(B / (med["fused"] * 1e-3), 1),
        "scorer_read_bytes": 4 * D * B * (2 + N),
        "loss": {k: v for k, v in losses.items() if v is not None},
        "conditions": {"fused_below_train": ok_c, "fused_below_module": ok_a},
    }
    text = json.dumps(line)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    return 0 if ok_c and ok_a else 1


if __name__ == "__main__":
    sys.exit(main())
