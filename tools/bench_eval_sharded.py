#!/usr/bin/env python3
"""Row-sharded exact retrieval at BASELINE config C3's shape, one rank of eight: rank 0 of an
emulated W = 8 job under MirrorComm (65,536 queries in total = 8,192 per rank, 2M x 96 items =
250K per rank, k = 80, 20 blocked items per query; synthetic embeddings, no model) against
one-process ``retrieve_topk`` at the full shape, alternating in one process after a warm-up of
both.

    python tools/bench_eval_sharded.py [--config c3|tiny] [--rounds 5] [--out profiles/eval_sharded_c3.json]

The rank does exactly the per-rank work of the W-rank job — the all-gathered W x 8,192 queries
scanned over its 250K-item shard, the blocked pairs grouped by owner, the W partial lists of its
own queries merged — with no interconnect traffic (MirrorComm hands the rank its own send chunks
back), so the stage times are device times of the local work and the exchanges' copies, not of a
fabric.  Each stage of ``retrieve_topk_program`` is bracketed by device events: gather, blocked
routing (two host syncs: the count matrix), shard scan, return exchange, merge.  The blocked ids
are built so that every owner gets the same number of pairs (MirrorComm's all-to-all needs the
mirrored splits to agree with the all-gathered counts).

MirrorComm's values are not those of a real job, so the tool checks shapes and id ranges only;
the exit status is 1 when they are wrong.  Prints one JSON line (and writes it to --out)."""

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
    "c3": dict(world=8, nq=65_536, ni=2_000_000, D=96, k=80, blocked=20),
    "tiny": dict(world=8, nq=1_024, ni=8_000, D=32, k=20, blocked=20),
}
STAGES = ("gather", "route_blocked", "scan", "return", "merge")


def blocked_lists(nq: int, nb: int, n_local: int, world: int, gen: torch.Generator, spread: bool
                  ) -> tuple[torch.Tensor, torch.Tensor]:
    """CSR of ``nb`` blocked global ids per query, ascending and distinct.  ``spread``: pair p of
    the rank goes to owner p % world (every owner gets the same count); else any item."""
    gaps = torch.randint(1, max(n_local // nb, 2), (nq, nb), generator=gen)
    rows = torch.cumsum(gaps, dim=1) - 1  # ascending distinct local rows < n_local
    if spread:
        owner = (torch.arange(nq * nb) % world).reshape(nq, nb)
        vals = rows * world + owner
    else:
        vals = rows * world + torch.randint(0, world, (nq, 1), generator=gen)
    return torch.arange(0, nb * nq + 1, nb), vals.reshape(-1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_sharded needs the MI355X (no CPU fallback)")
    from ttamm.retrieval import retrieve_topk
    from ttamm.sharded import MirrorComm, RowOwnership, retrieve_topk_program

    c = CONFIGS[args.config]
    W, nq, ni, D, k, nb = c["world"], c["nq"], c["ni"], c["D"], c["k"], c["blocked"]
    nq_r, ni_r = nq // W, ni // W
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    g = torch.Generator().manual_seed(args.seed + 1)
    items = torch.randn((ni, D), device=dev)
    queries = torch.randn((nq, D), device=dev)
    own = RowOwnership(W, 0)
    items_r = own.shard(items)
    queries_r = queries[:nq_r].contiguous()
    boff_r, bval_r = (t.to(dev) for t in blocked_lists(nq_r, nb, ni_r, W, g, spread=True))
    boff, bval = (t.to(dev) for t in blocked_lists(nq, nb, ni_r, W, g, spread=False))
    comm = MirrorComm(W, 0)

    def sharded():
        tl: list = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s, i = comm.run(retrieve_topk_program(own, queries_r, items_r, k, blocked_offsets=boff_r,
                                              blocked_values=bval_r, timeline=tl))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        stage = dict.fromkeys(STAGES, 0.0)
        for (_, a), (name, b) in zip(tl, tl[1:]):
            if name != "start":
                stage[name] += a.elapsed_time(b)
        return stage, wall, s, i

    def single():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        s, i = retrieve_topk(queries, items, k, blocked_offsets=boff, blocked_values=bval)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), s, i

    sharded()  # every code object and shape of the timed windows
    single()
    stages = {name: [] for name in STAGES}
    rank_ms, wall_ms, one_ms = [], [], []
    ok = True
    for _ in range(args.rounds):
        stage, wall, s, i = sharded()
        for name in STAGES:
            stages[name].append(stage[name])
        rank_ms.append(sum(stage.values()))
        wall_ms.append(wall)
        ok &= tuple(s.shape) == (nq_r, k) and tuple(i.shape) == (nq_r, k) and s.dtype == torch.float32
        ok &= i.dtype == torch.long and bool(((i >= -1) & (i < ni)).all())
        ms, s1, i1 = single()
        one_ms.append(ms)
        ok &= tuple(s1.shape) == (nq, k) and tuple(i1.shape) == (nq, k) and bool(((i1 >= -1) & (i1 < ni)).all())

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    med_rank, med_one = statistics.median(rank_ms), statistics.median(one_ms)
    med_stage = {name: statistics.median(v) for name, v in stages.items()}
    line = {
        "metric": "row-sharded exact top-k, rank 0 of an emulated 8-rank job (MirrorComm: local work and copies, no fabric) "
                  "vs one-process retrieve_topk at the full shape; device events, ms",
        "config": {"name": args.config, "world": W, "queries": nq, "queries_per_rank": nq_r, "items": ni,
                   "items_per_rank": ni_r, "dim": D, "k": k, "blocked_per_query": nb, "query_rounds": 1},
        "rounds": args.rounds,
        "stage_ms": {name: stat(v) for name, v in stages.items()},
        "per_rank_ms": stat(rank_ms),
        "per_rank_host_wall_ms": stat(wall_ms),
        "one_process_ms": stat(one_ms),
        "one_process_over_world_ms": round(med_one / W, 4),
        "per_rank_over_ideal_split": round(med_rank / (med_one / W), 3),
        "per_rank_over_one_process": round(med_rank / med_one, 4),
        "stage_share_of_per_rank": {name: round(v / med_rank, 4) for name, v in med_stage.items()},
        "merge_share_of_per_rank": round(med_stage["merge"] / med_rank, 4),
        "bytes_per_round_from_shapes": {"queries_gathered": W * nq_r * D * 4, "lists_returned": W * nq_r * k * 12,
                                        "blocked_pairs_sent": nq_r * nb * 16,
                                        "merge_kernel": W * nq_r * k * 12 + nq_r * k * 12},
        "merge_kernel_GBps": round((W + 1) * nq_r * k * 12 / (med_stage["merge"] * 1e-3) / 1e9, 2),
        "conditions": {"shapes_and_id_ranges": bool(ok)},
    }
    text = json.dumps(line)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
