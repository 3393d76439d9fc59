#!/usr/bin/env python3
"""In-batch scoring kernel benchmark (ttamm.inbatch_bce -> inbatch_x_kernel + ib_reduce_kernel).

    python tools/bench_inbatch.py [--batch 8192] [--positives 65536] [--dim 128] [--reps 20]
                                  [--loss {bce,softmax}] [--temperature T] [--row-base R] [--out FILE]

Default shape: one rank of the 8-rank C4 step (BASELINE configs[3]): 8192 users x the 65,536
all-gathered positives, D = 128.  Algorithmic work 6 B Bg D flops (S = U P^T, dU = dS P,
dP = dS^T U); the kernel forms S twice (user and item roles), so its split-bf16 ceiling for the
algorithmic flops is (2.5 PF / 6) x 6 / 8 = 312.5 TF/s.  Timed with HIP events on the launch
stream; the first launch is checked against the chunked fp64 oracle definition.

--loss softmax times the softmax objective (ttamm.inbatch_softmax: the LSE pass, the merge, the
softmax gradient kernel and the reduce; five score-sized products against BCE's four) and, in the
same process, its comparison points: the BCE op, the LSE pass alone (ttamm.inbatch_softmax_loss) and
ttamm.inbatch_bce_loss.  Every op is warmed up, then the four are timed in alternating rounds and the
per-launch median over the rounds is reported (the spread as min / max); --out appends the JSON
line's object to a JSON list in FILE."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

CEILING = 2500.0 / 6.0 * 6.0 / 8.0


def timed(fn, reps: int) -> float:
    """ms per call of fn over reps back-to-back calls (device events on the launch stream)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def bench_softmax(args, u, p, row_base: int) -> dict:
    import ttamm

    B, Bc, D = args.batch, args.positives, args.dim
    t = args.temperature
    ops = {
        "inbatch_bce": lambda: ttamm.inbatch_bce(u, p, row_base=row_base),
        "inbatch_softmax": lambda: ttamm.inbatch_softmax(u, p, row_base=row_base, temperature=t),
        "inbatch_softmax_loss": lambda: ttamm.inbatch_softmax_loss(u, p, row_base=row_base, temperature=t),
        "inbatch_bce_loss": lambda: ttamm.inbatch_bce_loss(u, p, row_base=row_base),
    }
    loss, du, dp = ops["inbatch_softmax"]()
    fwd = ops["inbatch_softmax_loss"]()
    torch.cuda.synchronize()
    err = None
    if not args.no_check:
        sys.path.insert(0, str(ROOT / "tests"))
        from softmax_reference import inbatch_softmax_chunked

        wl, wdu, wdp = inbatch_softmax_chunked(u, p, row_base=row_base, temperature=t)
        err = {"loss": abs(float(loss) - wl) / abs(wl),
               "dU": float((du.double() - wdu).abs().max() / wdu.abs().max()),
               "dP": float((dp.double() - wdp).abs().max() / wdp.abs().max()),
               "forward_only_bit_equal": float(fwd) == float(loss)}
    for fn in ops.values():  # warm every op at this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in ops}
    for _ in range(args.rounds):  # alternating: drift and neighbours hit every op alike
        for k, fn in ops.items():
            rounds[k].append(timed(fn, args.reps))
    out = {"B": B, "Bc": Bc, "D": D, "row_base": row_base, "temperature": t, "reps": args.reps,
           "rounds": args.rounds, "ms_per_launch": {}, "rel_err_vs_fp64": err}
    for k, v in rounds.items():
        v = sorted(v)
        out["ms_per_launch"][k] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    med = {k: v["median"] for k, v in out["ms_per_launch"].items()}
    out["softmax_over_bce"] = round(med["inbatch_softmax"] / med["inbatch_bce"], 4)
    out["lse_pass_share_of_softmax"] = round(med["inbatch_softmax_loss"] / med["inbatch_softmax"], 4)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--positives", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--loss", choices=("bce", "softmax"), default="bce")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--row-base", type=int, default=None, help="default: (positives - batch) // 2")
    ap.add_argument("--rounds", type=int, default=5, help="--loss softmax: alternating timing rounds")
    ap.add_argument("--out", type=Path, default=None, help="--loss softmax: append the result to this JSON list")
    args = ap.parse_args()
    import ttamm

    B, Bc, D = args.batch, args.positives, args.dim
    g = torch.Generator(device="cuda").manual_seed(11)
    u = torch.randn((B, D), device="cuda", generator=g) * 0.3
    p = torch.randn((Bc, D), device="cuda", generator=g) * 0.3
    row_base = (Bc - B) // 2 if args.row_base is None else args.row_base
    p[row_base:row_base + B] += 0.5 * u
    if args.loss == "softmax":
        res = bench_softmax(args, u, p, row_base)
        print(json.dumps(res), flush=True)
        if args.out is not None:
            prev = json.loads(args.out.read_text()) if args.out.exists() else []
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text(json.dumps(prev + [res], indent=1) + "\n")
        return
    inv = 1.0 / (Bc * Bc)
    loss, du, dp = ttamm.inbatch_bce(u, p, row_base=row_base, inv_count=inv)
    torch.cuda.synchronize()
    err = None
    if not args.no_check:
        from oracle import cpu_reference as ref

        wl, wdu, wdp = ref.inbatch_bce_chunked(u, p, row_base=row_base, inv_count=inv)
        err = {"loss": abs(float(loss) - wl) / abs(wl),
               "dU": float((du.double() - wdu).abs().max() / wdu.abs().max()),
               "dP": float((dp.double() - wdp).abs().max() / wdp.abs().max())}
    ms = timed(lambda: ttamm.inbatch_bce(u, p, row_base=row_base, inv_count=inv), args.reps)
    flops = 6.0 * B * Bc * D
    tf = flops / (ms * 1e-3) / 1e12
    print(json.dumps({"kernel": "inbatch_x_kernel + ib_reduce_kernel (ttamm_inbatch_bce)", "B": B, "Bc": Bc, "D": D,
                      "ms_per_launch": round(ms, 4), "achieved_tflops": round(tf, 2),
                      "peak": round(CEILING, 1), "frac": round(tf / CEILING, 4), "rel_err_vs_fp64": err}),
          flush=True)


if __name__ == "__main__":
    main()
