"""ttamm.topk_merge (ttamm_topk_merge, csrc/retrieval.hip) against numpy: per query a lexsort on
(-score, global id) of the entries that are not holes, global id = id * id_stride + list in
int64.  Scores come from four values, so ties are everywhere and the id order decides; outputs are
compared bit for bit."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import ttamm

pytestmark = pytest.mark.gpu

VALUES = np.array([-1.5, 0.25, 0.5, 3.0], dtype=np.float32)
QUERY_COUNTS = (1, 65, 130)  # one wave; one block of four and a wave; 32 blocks and a half
# n_lists, k_in, k_out: every boundary of the kernel's 512-slot rounds
SHAPES = [
    (1, 1, 1),       # smallest
    (1, 192, 192),   # plain re-sort
    (2, 20, 20),
    (3, 80, 80),
    (8, 64, 64),     # exactly 512 slots: one round
    (8, 65, 65),     # 520: the first shape with a second round
    (8, 192, 192),   # 1536 candidates, 320 new per round
    (64, 8, 192),    # many short lists
    (1024, 1, 5),    # the list limit
    (3, 5, 40),      # k_out above the candidates: a hole tail
]


def make_lists(rng: np.random.Generator, n_lists: int, nq: int, k_in: int, *, id_lo: int = 0, id_span: int = 5000,
               holes: float = 0.15) -> tuple[np.ndarray, np.ndarray]:
    """(scores, ids) [n_lists, nq, k_in]: unsorted lists, distinct ids per (list, query), holes (id
    -1, their scores kept finite) scattered inside them."""
    scores = VALUES[rng.integers(0, len(VALUES), size=(n_lists, nq, k_in))]
    # distinct per list: ascending with random gaps (all below id_span), then shuffled
    gaps = rng.integers(1, max(id_span // k_in, 1) + 1, size=(n_lists, nq, k_in), dtype=np.int64)
    ids = rng.permuted(id_lo + np.cumsum(gaps, axis=2) - 1, axis=2)
    ids[rng.random(ids.shape) < holes] = -1
    return scores, ids


def reference(scores: np.ndarray, ids: np.ndarray, k: int, id_stride: int) -> tuple[np.ndarray, np.ndarray]:
    n_lists, nq, k_in = scores.shape
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    lists = np.repeat(np.arange(n_lists, dtype=np.int64), k_in)
    for q in range(nq):
        s = scores[:, q, :].reshape(-1)
        i = ids[:, q, :].reshape(-1)
        keep = i >= 0
        g = (i * np.int64(id_stride) + lists)[keep]
        s = s[keep]
        order = np.lexsort((g, -s))[:k]
        out_s[q, :order.size] = s[order]
        out_i[q, :order.size] = g[order]
    return out_s, out_i


def run(scores: np.ndarray, ids: np.ndarray, k: int, id_stride: int = 1):
    s, i = ttamm.topk_merge(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda(), k, id_stride=id_stride)
    return s.cpu().numpy(), i.cpu().numpy()


def check(scores: np.ndarray, ids: np.ndarray, k: int, id_stride: int, got=None) -> None:
    got_s, got_i = got if got is not None else run(scores, ids, k, id_stride)
    want_s, want_i = reference(scores, ids, k, id_stride)
    assert got_s.shape == want_s.shape and got_i.shape == want_i.shape
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32))


@pytest.mark.parametrize("n_lists,k_in,k_out", SHAPES, ids=[f"{a}x{b}to{c}" for a, b, c in SHAPES])
def test_merge_matches_lexsort(n_lists, k_in, k_out):
    rng = np.random.default_rng(1000 * n_lists + k_in)
    for nq in QUERY_COUNTS:
        scores, ids = make_lists(rng, n_lists, nq, k_in)
        stride = 1 if n_lists == 1 else n_lists
        check(scores, ids, k_out, stride)


def test_whole_lists_of_holes_and_all_hole_queries():
    rng = np.random.default_rng(7)
    scores, ids = make_lists(rng, 8, 65, 80)
    ids[3] = -1           # one list empty for every query
    ids[:, 5] = -1        # query 5: nothing at all
    ids[1:, 6] = -1       # query 6: one list only
    ids[:, 64, 1:] = -1   # the last query: one entry per list
    ids[:, 64, 0] = 100 + np.arange(8)
    got_s, got_i = run(scores, ids, 80, 8)
    check(scores, ids, 80, 8, got=(got_s, got_i))
    assert (got_i[5] == -1).all() and np.isneginf(got_s[5]).all()
    assert (got_i[64, 8:] == -1).all() and (got_i[64, :8] >= 0).all()


def test_hole_scores_are_ignored():
    """A hole is a hole whatever its score: +inf on a hole must not surface, and a real entry
    with score -inf still comes before the holes."""
    scores = np.array([[[np.inf, 1.0, -np.inf]], [[2.0, np.inf, 0.0]]], dtype=np.float32)
    ids = np.array([[[-1, 4, 9]], [[7, -5, -1]]], dtype=np.int64)
    got_s, got_i = run(scores, ids, 5, 2)
    assert got_i.tolist() == [[15, 8, 18, -1, -1]]
    assert got_s.tolist() == [[2.0, 1.0, -np.inf, -np.inf, -np.inf]]


def test_global_ids_past_2_to_31_are_compared_in_64_bits():
    """id_stride = 8 with local ids around 2^28 and 2^29: the global ids straddle 2^31 (where a
    signed 32-bit compare flips) and 2^32 (where a truncated one wraps)."""
    rng = np.random.default_rng(11)
    nq, k_in = 65, 48
    s_lo, i_lo = make_lists(rng, 8, nq, k_in, id_lo=2 ** 28 - 60, id_span=120, holes=0.05)
    s_hi, i_hi = make_lists(rng, 8, nq, k_in, id_lo=2 ** 29 - 60, id_span=120, holes=0.05)
    scores = np.concatenate([s_lo, s_hi], axis=2)
    ids = np.concatenate([i_lo, i_hi], axis=2)
    got = run(scores, ids, 192, 8)
    check(scores, ids, 192, 8, got=got)
    real = got[1][got[1] >= 0]
    assert (real < 2 ** 31).any() and (real >= 2 ** 31).any() and (real >= 2 ** 32).any()


def test_strided_views_of_a_larger_buffer():
    rng = np.random.default_rng(13)
    n_lists, nq, k_in = 5, 65, 30
    scores, ids = make_lists(rng, n_lists, nq, k_in)
    big_s = torch.full((n_lists + 1, 2 * nq + 3, k_in + 7), float("nan"), device="cuda")
    big_i = torch.full((n_lists + 1, 2 * nq + 3, k_in + 7), 123456, dtype=torch.long, device="cuda")
    view_s = big_s[1:, 1:1 + 2 * nq:2, 3:3 + k_in]
    view_i = big_i[1:, 1:1 + 2 * nq:2, 3:3 + k_in]
    view_s.copy_(torch.from_numpy(scores))
    view_i.copy_(torch.from_numpy(ids))
    assert not view_s.is_contiguous() and view_s.stride() == view_i.stride()
    s, i = ttamm.topk_merge(view_s, view_i, 30, id_stride=n_lists)
    check(scores, ids, 30, n_lists, got=(s.cpu().numpy(), i.cpu().numpy()))


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(17)
    scores, ids = make_lists(rng, 8, 130, 192)
    s = torch.from_numpy(scores).cuda()
    i = torch.from_numpy(ids).cuda()
    a = ttamm.topk_merge(s, i, 192, id_stride=8)
    b = ttamm.topk_merge(s, i, 192, id_stride=8)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_zero_queries_launch_nothing():
    s, i = ttamm.topk_merge(torch.empty((3, 0, 8), device="cuda"), torch.empty((3, 0, 8), dtype=torch.long, device="cuda"), 8)
    assert s.shape == (0, 8) and i.shape == (0, 8)


@pytest.mark.parametrize("n_lists,k_in,k_out,id_stride", [(1, 4, 193, 1), (1025, 1, 1, 1), (2, 4, 4, 0), (1, 4, 0, 1)],
                         ids=["k_out-193", "n_lists-1025", "id_stride-0", "k_out-0"])
def test_launcher_rejects_bad_arguments(n_lists, k_in, k_out, id_stride):
    s = torch.zeros((n_lists, 2, k_in), device="cuda")
    i = torch.zeros((n_lists, 2, k_in), dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="topk_merge"):
        ttamm.topk_merge(s, i, k_out, id_stride=id_stride)


def test_k_in_above_192_is_rejected():
    s = torch.zeros((1, 1, 193), device="cuda")
    with pytest.raises(ValueError, match="topk_merge"):
        ttamm.topk_merge(s, torch.zeros((1, 1, 193), dtype=torch.long, device="cuda"), 4)
