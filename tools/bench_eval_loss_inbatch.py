#!/usr/bin/env python3
"""In-batch validation at BASELINE config C2 (B = Bc = 8192, D = 96; tables and towers as C2, N = 5):
four things timed in one process, alternating, device events around each window of launches after
a warm-up of every variant:

  (a) op_full:   `ttamm.inbatch_bce`, the training kernel (both roles, dU, dP, slabs, the reduce);
  (b) op_loss:   `ttamm.inbatch_bce_loss`, the forward-only inbatch_loss_kernel, on the same rows;
  (c) eval_step: `FusedEvalLoss(in_batch_negatives=True).step` (one `ttamm_eval_loss_inbatch` per batch);
  (d) train:     `FusedTrainStep(in_batch_negatives=True).step` on the same batches.

    python tools/bench_eval_loss_inbatch.py [--config c2] [--batches 50] [--launches 50] [--rounds 5] [--out FILE]

The op windows include the ops' output / workspace allocations (both variants alike).  (b) is also
checked against the chunked float64 value at the same shape (<= 1e-5 relative; the error is
recorded).  Prints one JSON line (and writes it to --out): the median over the rounds of each
variant with its min / max, the kernel's executed bf16 MFMA flops 2 * 5 * B * Bc * D and bytes
4 * D * (B + rblk * Bc) from shapes, and the op's rates: executed bf16 TF/s against the 2.5 PF/s
MFMA peak, and the fp32 product 2 * B * Bc * D against the 416.7 TF/s split-bf16 ceiling that
DESIGN prices every split kernel with (the window holds the op's allocations and its
256-thread sum launch too, so the kernel alone is at least this fast).
Gates (exit status 1 if one fails): (b) < 0.5 x (a) — (b) does 1/6 of (a)'s MFMA products and
1/2 of its elementwise passes, no slab write and no reduce launch — (c) < (d): the pass runs a
strict subset of the step's work — and the float64 check."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"))

import torch  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0
CEILING_TFLOPS = 416.7  # split-bf16 ceiling of DESIGN: 2.5 PF/s bf16 / 6 MFMAs per fp32 product


def timed(fn) -> float:
    """Device ms of fn(), events on the current stream, synchronised."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "tiny"])
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_loss_inbatch needs the MI355X (no CPU fallback)")
    import bench
    import ttamm
    from oracle import cpu_reference as ref

    c = bench.CONFIGS[args.config]
    dev = torch.device("cuda")
    B, N, D = c["B"], c["N"], c["D"]

    # ---- the op: (a) and (b) on the same rows -------------------------------------------------
    g = torch.Generator(device="cuda").manual_seed(args.seed + 1)
    users = torch.randn((B, D), device=dev, generator=g) * 0.3
    pos = torch.randn((B, D), device=dev, generator=g) * 0.3
    pos += 0.5 * users
    want, _, _ = ref.inbatch_bce_chunked(users, pos)
    got = float(ttamm.inbatch_bce_loss(users, pos))
    op_err = abs(got - want) / abs(want)

    def run_full():
        for _ in range(args.launches):
            ttamm.inbatch_bce(users, pos)

    def run_loss():
        for _ in range(args.launches):
            ttamm.inbatch_bce_loss(users, pos)

    # ---- the pass: (c) and (d) on the same batches --------------------------------------------
    w = bench.Workload(c, dev, args.seed, in_batch=True)
    K = args.batches
    batches = [w.batch() for _ in range(K)]
    engine = ttamm.FusedEvalLoss(w.model, negatives_per_positive=N, positives=w.csr, user_features=w.user_features,
                                 item_features=w.item_features, max_batch=B, seed=args.seed,
                                 in_batch_negatives=True)
    losses = {}

    def run_eval(bs=batches):
        for u, p in bs:
            engine.step(u, p)

    def run_train(bs=batches):
        for u, p in bs:
            w.engine.step(u, p)

    for _ in range(2):  # every shape and code object of the timed windows
        run_full()
        run_loss()
    run_eval(batches[: args.warmup])
    engine.finish()
    run_train(batches[: args.warmup])
    w.engine.flush()
    torch.cuda.synchronize()

    ms = {"op_full": [], "op_loss": [], "eval_step": [], "train": []}
    for _ in range(args.rounds):
        ms["op_full"].append(timed(run_full) / args.launches)
        ms["op_loss"].append(timed(run_loss) / args.launches)
        ms["eval_step"].append(timed(run_eval) / K)
        losses["eval_step"] = engine.finish()
        ms["train"].append(timed(run_train) / K)
        w.engine.flush()  # outside the window: the deferred tables brought current for the pass
    w.engine.finish()

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    med = {k: statistics.median(v) for k, v in ms.items()}
    rblk = -(-B // 256)
    flops = 2 * 5 * B * B * D
    ok_b, ok_c, ok_err = med["op_loss"] < 0.5 * med["op_full"], med["eval_step"] < med["train"], op_err <= 1e-5
    tflops = flops / (med["op_loss"] * 1e-3) / 1e12
    alg_tflops = tflops / 5
    line = {
        "metric": "in-batch validation, ms per launch / per batch (device events around windows)",
        "config": {"name": args.config, **{k: c[k] for k in ("U", "I", "F", "H", "D", "B", "N")}},
        "launches": args.launches, "batches": K, "rounds": args.rounds, "warmup_batches": args.warmup,
        "ms": {k: stat(v) for k, v in ms.items()},
        "op_loss_over_op_full": round(med["op_loss"] / med["op_full"], 3),
        "eval_step_over_train": round(med["eval_step"] / med["train"], 3),
        "op_loss_rel_err_vs_fp64": op_err,
        "kernel_mfma_flops": flops,
        "kernel_bytes": 4 * D * (B + rblk * B),
        "op_loss_bf16_mfma_tflops": round(tflops, 1),
        "op_loss_fraction_of_bf16_mfma_peak": round(tflops / BF16_PEAK_TFLOPS, 3),
        "op_loss_fp32_product_tflops": round(alg_tflops, 1),
        "op_loss_fraction_of_split_bf16_ceiling": round(alg_tflops / CEILING_TFLOPS, 3),
        "loss": losses,
        "conditions": {"op_loss_below_half_op_full": ok_b, "eval_step_below_train": ok_c, "op_loss_within_1e-5": ok_err},
    }
    text = json.dumps(line)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    return 0 if ok_b and ok_c and ok_err else 1


if __name__ == "__main__":
    sys.exit(main())
