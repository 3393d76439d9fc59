"""The row-sharded evaluation's exchange layer without a GPU: ``route_blocked`` (ttamm/sharded_eval.py)
under run_loopback with CPU tensors and the CPU router (oracle/route.py stands in for
ttamm_route_rows, as in tests/test_sharded_cpu.py) — every owner must end up with exactly the
blocked pairs of the items it owns, as a CSR over the round's W qb query slots, local rows
ascending per slot.  And the ABI constant the new entry point bumps."""

from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.route import route_rows
from ttamm import _lib
from ttamm.sharded import RowOwnership, retrieve_topk_program, route_blocked, run_loopback

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ttamm.h"


def _blocks(W: int, qb: int, counts: list[int], lengths, num_items: int, seed: int):
    """Per rank: (offsets [n + 1], values) of its n = counts[rank] <= qb queries, list lengths drawn
    from ``lengths``, global item ids ascending and unique per query."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(W):
        lens = [int(rng.choice(lengths)) for _ in range(counts[r])]
        vals = [np.sort(rng.choice(num_items, size=n, replace=False)) for n in lens]
        off = np.zeros(counts[r] + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        flat = np.concatenate(vals) if vals else np.zeros(0, dtype=np.int64)
        out.append((torch.from_numpy(off), torch.from_numpy(flat.astype(np.int64))))
    return out


def _expected(W: int, qb: int, blocks, owner: int):
    """numpy restatement: filter by % W, divide by W, group by slot (rank-major slots)."""
    per_slot = [np.zeros(0, dtype=np.int64) for _ in range(W * qb)]
    for r, (off, val) in enumerate(blocks):
        off, val = off.numpy(), val.numpy()
        for j in range(off.size - 1):
            v = val[off[j]:off[j + 1]]
            per_slot[r * qb + j] = v[v % W == owner] // W
    offsets = np.zeros(W * qb + 1, dtype=np.int64)
    np.cumsum([v.size for v in per_slot], out=offsets[1:])
    return offsets, np.concatenate(per_slot)


def _run(W: int, qb: int, blocks):
    def prog(r):
        off, val = blocks[r]
        return (yield from route_blocked(RowOwnership(W, r), route_rows, off, val, r * qb, W * qb))

    return run_loopback([prog(r) for r in range(W)])


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_route_blocked_owner_csr(W):
    qb = 7
    counts = [(qb - r) if r % 2 == 0 else max(qb - 2 * r, 1) for r in range(W)]
    blocks = _blocks(W, qb, counts, lengths=(0, 5, 100), num_items=403, seed=W)
    outs = _run(W, qb, blocks)
    for owner, (offsets, values) in enumerate(outs):
        want_off, want_val = _expected(W, qb, blocks, owner)
        assert offsets.dtype == torch.long and values.dtype == torch.long
        assert np.array_equal(offsets.numpy(), want_off)
        assert np.array_equal(values.numpy(), want_val)
        for s in range(W * qb):  # ascending and unique within each slot
            seg = values[offsets[s]:offsets[s + 1]]
            assert bool((seg[1:] > seg[:-1]).all())


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_route_blocked_empty_lists_and_empty_ranks(W):
    """Ranks without queries (an offsets tensor of one entry), queries without blocked items, and
    a world in which nothing is blocked at all."""
    qb = 4
    counts = [0 if r % 2 == 1 else qb for r in range(W)]
    if W == 1:
        counts = [3]
    blocks = _blocks(W, qb, counts, lengths=(0, 0, 9), num_items=50, seed=10 + W)
    for owner, (offsets, values) in enumerate(_run(W, qb, blocks)):
        want_off, want_val = _expected(W, qb, blocks, owner)
        assert np.array_equal(offsets.numpy(), want_off) and np.array_equal(values.numpy(), want_val)
    nothing = [(torch.zeros(c + 1, dtype=torch.long), torch.zeros(0, dtype=torch.long)) for c in counts]
    for offsets, values in _run(W, qb, nothing):
        assert offsets.tolist() == [0] * (W * qb + 1) and values.numel() == 0


def test_route_blocked_takes_a_slice_of_a_larger_csr():
    """A round's block is offsets[lo:hi + 1] over the rank's whole value array."""
    W, qb = 2, 3
    whole = _blocks(W, 8, [8, 8], lengths=(2, 5), num_items=60, seed=3)
    sliced = [(off[2:2 + qb + 1], val) for off, val in whole]
    rebased = [(off[2:2 + qb + 1] - off[2], val[int(off[2]):int(off[2 + qb])]) for off, val in whole]
    for owner, (offsets, values) in enumerate(_run(W, qb, sliced)):
        want_off, want_val = _expected(W, qb, rebased, owner)
        assert np.array_equal(offsets.numpy(), want_off) and np.array_equal(values.numpy(), want_val)


def test_entry_points_are_exported():
    import ttamm
    from ttamm import sharded

    assert "topk_merge" in ttamm.__all__ and callable(ttamm.topk_merge)
    for name in ("evaluate_metrics_sharded", "evaluate_metrics_program", "retrieve_topk_program", "route_blocked"):
        assert callable(getattr(sharded, name))
    assert retrieve_topk_program is sharded.retrieve_topk_program
    assert "ttamm_topk_merge" in _lib.SIGNATURES


def test_sampled_branch_is_refused_before_any_collective():
    from ttamm.sharded import evaluate_metrics_program

    with pytest.raises(NotImplementedError):
        evaluate_metrics_program(None, RowOwnership(2, 0), train_positive_map={}, val_interactions=[],
                                 item_feature_tensor=None, user_feature_tensor=None, num_items=10,
                                 rng=np.random.default_rng(0), candidate_samples=5)


def test_abi_version_is_29(tmp_path):
    assert _lib.ABI_VERSION == 29
    src = tmp_path / "abi.c"
    src.write_text(f'#include "{HEADER}"\nint main(void) {{ return TTAMM_ABI_VERSION == 29 ? 0 : 1; }}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(tmp_path / "abi")], check=True)
    subprocess.run([str(tmp_path / "abi")], check=True)
    assert _lib.load().ttamm_abi_version() == 29
