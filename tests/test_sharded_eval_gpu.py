"""The row-sharded evaluation (ttamm/sharded_eval.py) on one GPU: W virtual ranks run in lock step
under run_loopback, each with its item shard and its own queries.

a) exact arithmetic — embeddings from {-2, ..., 2} / 4: every product and every sum is exact in
   the bf16 planes and in fp32, so the ranks' concatenated (scores, ids) must equal a numpy int64
   oracle (integer scores x 1/16, blocked items removed, lexsort on (-score, id)) bit for bit,
   cross-rank tie order included, and one-process ``retrieve_topk`` on the global matrix;
b) random normal embeddings — bit-equal to one-process ``retrieve_topk``: a pair's arithmetic
   does not depend on where the item sits in a tile or partition;
c) end to end — sharded models built as tests/test_sharded_gpu.py builds its ranks:
   ``evaluate_metrics_program`` against ``ranking_metrics`` of one-process ``retrieve_topk`` over
   the reassembled embeddings."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest
import torch
from torch import nn

import ttamm
from helpers import Shape, make_problem, rel_err
from ttamm.metrics import truth_csr
from ttamm.retrieval import (blocked_csr, encode_item_embeddings, encode_user_embeddings, normalize_rows,
                             retrieve_topk)
from ttamm.samplers import PositivesCSR
from ttamm.sharded import (RowOwnership, evaluate_metrics_program, evaluate_metrics_sharded, retrieve_topk_program,
                           run_loopback)

pytestmark = pytest.mark.gpu

WORLDS = [(1, 900), (2, 901), (3, 1000), (8, 1003)]  # (W, items): unequal shards
COUNTS = {1: [70], 2: [70, 0], 3: [70, 0, 33], 8: [70, 0, 33, 5, 64, 65, 1, 12]}  # queries per rank
LENGTHS = (0, 5, 100)  # blocked items per query, in turn; 100 spans every owner and takes the binary search


@dataclasses.dataclass
class Case:
    W: int
    items: torch.Tensor  # [I, D] global, on the device
    queries: list  # per rank [n_r, D]
    boff: list  # per rank CSR offsets over its queries
    bval: list  # per rank global blocked ids, ascending per query
    blocked: list  # per global query (rank-major) a numpy array


def _make(W: int, I: int, D: int, counts, lengths, exact: bool, seed: int) -> Case:
    rng = np.random.default_rng(seed)

    def draw(n):
        if exact:
            return (rng.integers(-2, 3, size=(n, D)).astype(np.float32)) / 4
        return rng.standard_normal((n, D)).astype(np.float32)

    items = torch.from_numpy(draw(I)).cuda()
    queries, boff, bval, blocked = [], [], [], []
    j = 0
    for r in range(W):
        queries.append(torch.from_numpy(draw(counts[r])).cuda())
        off, vals = [0], []
        for _ in range(counts[r]):
            b = np.sort(rng.choice(I, size=min(lengths[j % len(lengths)], I), replace=False)).astype(np.int64)
            j += 1
            blocked.append(b)
            vals.append(b)
            off.append(off[-1] + b.size)
        boff.append(torch.tensor(off, dtype=torch.long, device="cuda"))
        bval.append(torch.from_numpy(np.concatenate(vals) if vals else np.zeros(0, dtype=np.int64)).cuda())
    return Case(W, items, queries, boff, bval, blocked)


@functools.lru_cache(maxsize=None)
def exact_case(W: int, I: int, D: int) -> Case:
    return _make(W, I, D, COUNTS[W], LENGTHS, True, 1000 * W + D)


@functools.lru_cache(maxsize=None)
def random_case(W: int, I: int, D: int) -> Case:
    return _make(W, I, D, COUNTS[W], LENGTHS, False, 2000 * W + D)


@functools.lru_cache(maxsize=None)
def short_case() -> Case:
    """40 items over 8 ranks, 20 or 25 of them blocked per query: shards of 5 items return holes
    at k = 20 and the global list of every other query is short."""
    return _make(8, 40, 32, [9, 0, 4, 7, 1, 3, 2, 5], (20, 25), True, 99)


def int_oracle(case: Case, k: int) -> tuple[np.ndarray, np.ndarray]:
    """numpy int64: integer scores x 1/16, blocked removed, lexsort on (-score, id)."""
    x = np.rint(case.items.cpu().numpy() * 4).astype(np.int64)
    q = np.rint(torch.cat(case.queries).cpu().numpy() * 4).astype(np.int64)
    s = q @ x.T
    out_s = np.full((q.shape[0], k), -np.inf, dtype=np.float32)
    out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
    ids = np.arange(x.shape[0], dtype=np.int64)
    for j in range(q.shape[0]):
        keep = np.ones(x.shape[0], dtype=bool)
        keep[case.blocked[j]] = False
        cand = ids[keep]
        order = cand[np.lexsort((cand, -s[j, cand]))][:k]
        out_i[j, :order.size] = order
        out_s[j, :order.size] = (s[j, order].astype(np.float64) / 16).astype(np.float32)
    return out_s, out_i


def one_process(case: Case, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    off = [torch.zeros(1, dtype=torch.long, device="cuda")]
    base = 0
    for o, v in zip(case.boff, case.bval):
        off.append(o[1:] + base)
        base += v.numel()
    return retrieve_topk(torch.cat(case.queries), case.items, k, blocked_offsets=torch.cat(off),
                         blocked_values=torch.cat(case.bval))


def sharded(case: Case, k: int, query_block: int) -> tuple[torch.Tensor, torch.Tensor]:
    W = case.W
    progs = [retrieve_topk_program(RowOwnership(W, r), case.queries[r], RowOwnership(W, r).shard(case.items), k,
                                   blocked_offsets=case.boff[r], blocked_values=case.bval[r], query_block=query_block)
             for r in range(W)]
    outs = run_loopback(progs)
    for r, (s, i) in enumerate(outs):
        assert s.shape == (case.queries[r].shape[0], k) and i.shape == s.shape
    return torch.cat([s for s, _ in outs]), torch.cat([i for _, i in outs])


def assert_same_bits(got, want_s, want_i) -> None:
    s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_s = want_s.cpu().numpy() if torch.is_tensor(want_s) else want_s
    want_i = want_i.cpu().numpy() if torch.is_tensor(want_i) else want_i
    assert np.array_equal(i, want_i)
    assert np.array_equal(s.view(np.int32), want_s.view(np.int32))


@pytest.mark.parametrize("query_block", [64, 65536])
@pytest.mark.parametrize("k", [1, 20, 192])
@pytest.mark.parametrize("W,I", WORLDS)
@pytest.mark.parametrize("D", [32, 96, 200])  # 200 takes the fp32 kernel
def test_exact_arithmetic_matches_int_oracle(D, W, I, k, query_block):
    case = exact_case(W, I, D)
    got = sharded(case, k, query_block)
    assert_same_bits(got, *int_oracle(case, k))
    assert_same_bits(got, *one_process(case, k))


@pytest.mark.parametrize("query_block", [3, 65536])
def test_short_global_lists_and_shards_that_return_holes(query_block):
    case = short_case()
    got = sharded(case, 20, query_block)
    want_s, want_i = int_oracle(case, 20)
    assert (want_i[:, 15:] == -1).any() and (want_i[:, :15] >= 0).all()
    assert_same_bits(got, want_s, want_i)
    assert_same_bits(got, *one_process(case, 20))


def test_no_blocked_lists_at_all():
    """No rank passes a blocked CSR: no routing round, same result."""
    case = exact_case(3, 1000, 96)
    bare = dataclasses.replace(case, boff=[None] * 3, bval=[None] * 3,
                               blocked=[np.zeros(0, dtype=np.int64)] * len(case.blocked))
    got = sharded(bare, 20, 64)
    assert_same_bits(got, *int_oracle(bare, 20))


@pytest.mark.parametrize("query_block", [64, 65536])
@pytest.mark.parametrize("k", [1, 20, 192])
@pytest.mark.parametrize("W,I", [(2, 901), (8, 1003)])
def test_random_embeddings_match_one_process_bits(W, I, k, query_block):
    case = random_case(W, I, 96)
    assert_same_bits(sharded(case, k, query_block), *one_process(case, k))


# ---------------------------------------------------------------------------------------
# c) end to end
# ---------------------------------------------------------------------------------------
TABLES = ("user_encoder.embedding.weight", "item_encoder.embedding.weight",
          "adaptive_mimic.user_augmented.weight", "adaptive_mimic.item_augmented.weight")
KS = (5, 20)


def _model(shape: Shape, U: int, I: int, state: dict, cosine: bool):
    cfg = shape.tower_cfg()
    ue = ttamm.build_tower_encoder(cfg, num_embeddings=U, feature_dim=shape.F, device="cuda")
    ie = ttamm.build_tower_encoder(cfg, num_embeddings=I, feature_dim=shape.F, device="cuda")
    mm = ttamm.AdaptiveMimicMechanism(num_users=U, num_items=I, embedding_dim=shape.D).cuda() if shape.mimic else None
    sim = nn.CosineSimilarity(dim=-1) if cosine else ttamm.DotProductSimilarity()
    m = ttamm.TwoTowerModel(ue, ie, similarity=sim, adaptive_mimic=mm)
    m.load_state_dict({k: v.cuda() for k, v in state.items()}, strict=True)
    return m


@dataclasses.dataclass
class World:
    shape: Shape
    W: int
    prob: object
    gm: object
    ranks: list  # (own, model, user features, item features, local positives)
    items: torch.Tensor  # reassembled [I, D] (normalised for a cosine model)
    pairs: torch.Tensor  # global (user, item) validation pairs
    rank_pairs: list  # per rank (local user row, global item)
    want: object  # one-process RankingMetrics with per-user rows
    users: torch.Tensor  # the reference's users, ascending


@functools.lru_cache(maxsize=None)
def world(W: int, cosine: bool) -> World:
    shape = Shape()
    prob = make_problem(shape, seed=77)
    state = prob.model.state_dict()
    gm = _model(shape, shape.U, shape.I, state, cosine).eval()
    ranks = []
    for r in range(W):
        own = RowOwnership(W, r)
        st = {k: (own.shard(v) if k in TABLES else v.clone()) for k, v in state.items()}
        m = _model(shape, own.local_count(shape.U), own.local_count(shape.I), st, cosine)
        local_pos = {u // W: prob.positives[u] for u in range(r, shape.U, W)}
        ranks.append((own, m, own.shard(prob.user_features).cuda(), own.shard(prob.item_features).cuda(), local_pos))
    # the ranks' item shards, reassembled, against the one-process encoding
    dev = torch.device("cuda")
    full = encode_item_embeddings(gm, num_items=shape.I, item_features=prob.item_features.cuda(), device=dev)
    items = torch.empty_like(full)
    for own, m, _, feats, _ in ranks:
        m.eval()
        items[own.rank::W] = encode_item_embeddings(m, num_items=own.local_count(shape.I), item_features=feats, device=dev)
    assert rel_err(items, full) <= 1e-6
    if cosine:
        normalize_rows(items)
    # validation pairs: users 0, 1, 2, 4, 5, 6, ... (every fourth has none), two items of each user's
    # one-process top-20 and one other item, so that hits occur
    users = torch.tensor([u for u in range(shape.U) if u % 4 != 3], dtype=torch.long, device=dev)
    q = _queries(ranks, W, users, prob, cosine, gm)
    boff, bval = blocked_csr(users.tolist(), prob.positives, dev)
    _, top = retrieve_topk(q, items, 20, blocked_offsets=boff, blocked_values=bval)
    g = torch.Generator().manual_seed(5)
    other = torch.randint(0, shape.I, (users.numel(), 1), generator=g).to(dev)
    chosen = torch.cat([top[:, [1, 7]], other], dim=1)
    pairs = torch.stack([users[:, None].expand_as(chosen).reshape(-1), chosen.reshape(-1)], dim=1)
    pairs = pairs[torch.randperm(pairs.shape[0], generator=g).to(dev)]
    rank_pairs = []
    for r in range(W):
        mine = pairs[pairs[:, 0] % W == r]
        rank_pairs.append(torch.stack([mine[:, 0] // W, mine[:, 1]], dim=1))
    tu, toff, tval = truth_csr(pairs)
    assert torch.equal(tu, users)
    _, ids = retrieve_topk(q, items, max(KS), blocked_offsets=boff, blocked_values=bval)
    want = ttamm.ranking_metrics(ids, toff, tval, KS, pad_with_truth=True, per_user=True)
    return World(shape, W, prob, gm, ranks, items, pairs, rank_pairs, want, users)


def _queries(ranks, W, users, prob, cosine, gm) -> torch.Tensor:
    """The ranks' encoded queries for the global ``users``, reassembled in their order, checked
    against the one-process user tower."""
    q = None
    for own, m, ufeat, _, _ in ranks:
        mine = users % W == own.rank
        part = encode_user_embeddings(m, users[mine] // W, user_features=ufeat)
        if q is None:
            q = torch.empty((users.numel(), part.shape[1]), dtype=torch.float32, device=users.device)
        q[mine] = part
    full = encode_user_embeddings(gm, users, user_features=prob.user_features.cuda())
    assert rel_err(q, full) <= 1e-6
    if cosine:
        normalize_rows(q)
    return q


def _programs(w: World, *, pairs=None, per_user=False, csr=False, **kw):
    progs = []
    for (own, m, ufeat, ifeat, local_pos), rp in zip(w.ranks, pairs if pairs is not None else w.rank_pairs):
        pos = PositivesCSR.from_mapping(local_pos, device=torch.device("cuda")) if csr else local_pos
        progs.append(evaluate_metrics_program(m, own, train_positive_map=pos, val_interactions=rp,
                                              item_feature_tensor=ifeat, user_feature_tensor=ufeat,
                                              num_items=w.shape.I, k_values=KS, per_user=per_user, **kw))
    return progs


def _close(got, want) -> None:
    for name in ("recall", "precision", "ndcg", "hit_rate", "map"):
        for k in KS:
            a, b = getattr(got, name)[k], getattr(want, name)[k]
            assert abs(a - b) <= 1e-12 * abs(b), (name, k, a, b)
    assert abs(got.mrr - want.mrr) <= 1e-12 * abs(want.mrr)


@pytest.mark.parametrize("W,cosine,csr,query_block", [(2, False, False, 65536), (3, False, True, 7), (3, True, False, 65536),
                                                      (2, True, True, 65536)],
                         ids=["w2-dot", "w3-dot-csr-rounds", "w3-cosine", "w2-cosine-csr"])
def test_metrics_match_one_process(W, cosine, csr, query_block):
    w = world(W, cosine)
    assert w.want.recall[20] > 0  # the pairs were chosen so that hits occur
    outs = run_loopback(_programs(w, csr=csr, query_block=query_block))
    for got in outs:
        _close(got, w.want)
        assert got == outs[0] and got.per_user == []  # every rank: identical values


@pytest.mark.parametrize("W", [2, 3])
def test_per_user_rows_are_the_ranks_own_users(W):
    w = world(W, False)
    outs = run_loopback(_programs(w, per_user=True))
    users = w.users.tolist()
    for r, got in enumerate(outs):
        _close(got, w.want)
        mine = [row for u, row in zip(users, w.want.per_user) if u % W == r]  # ascending local rows
        assert got.per_user == mine and len(mine) > 0
        assert dataclasses.replace(got, per_user=[]) == dataclasses.replace(outs[0], per_user=[])


def test_a_rank_without_pairs_and_precomputed_item_embeddings():
    """Rank 1 has no validation pair (it still serves its item shard); the ranks pass their
    already encoded shards."""
    W = 3
    w = world(W, False)
    keep = w.pairs[w.pairs[:, 0] % W != 1]
    pairs = [torch.stack([keep[keep[:, 0] % W == r][:, 0] // W, keep[keep[:, 0] % W == r][:, 1]], dim=1) for r in range(W)]
    assert pairs[1].shape[0] == 0
    users, toff, tval = truth_csr(keep)
    q = _queries(w.ranks, W, users, w.prob, False, w.gm)
    boff, bval = blocked_csr(users.tolist(), w.prob.positives, torch.device("cuda"))
    _, ids = retrieve_topk(q, w.items, max(KS), blocked_offsets=boff, blocked_values=bval)
    want = ttamm.ranking_metrics(ids, toff, tval, KS, pad_with_truth=True)
    progs = []
    for (own, m, ufeat, ifeat, local_pos), rp in zip(w.ranks, pairs):
        progs.append(evaluate_metrics_program(m, own, train_positive_map=local_pos, val_interactions=rp,
                                              item_feature_tensor=None, user_feature_tensor=ufeat,
                                              num_items=w.shape.I, k_values=KS,
                                              item_embeddings=w.items[own.rank::W].contiguous()))
    outs = run_loopback(progs)
    for got in outs:
        _close(got, want)
        assert got == outs[0]


@pytest.mark.parametrize("W", [1, 2, 3])
def test_a_world_without_validation_pairs_returns_zeros(W):
    w = world(max(W, 2), False)
    if W == 1:  # rank 0's shard of the two-rank world, taken as a whole one-rank model
        own, m, ufeat, ifeat, local_pos = w.ranks[0]
        outs = run_loopback([evaluate_metrics_program(
            m, RowOwnership(1, 0), train_positive_map=local_pos, val_interactions=torch.zeros((0, 2), dtype=torch.long),
            item_feature_tensor=ifeat, user_feature_tensor=ufeat, num_items=m.item_encoder.num_embeddings, k_values=KS)])
    else:
        empty = [torch.zeros((0, 2), dtype=torch.long, device="cuda") for _ in range(W)]
        outs = run_loopback(_programs(w, pairs=empty))
    for got in outs:
        assert got.mrr == 0.0 and got.per_user == []
        assert all(v == 0.0 for name in ("recall", "precision", "ndcg", "hit_rate", "map")
                   for v in getattr(got, name).values())
        assert set(got.recall) == set(KS)


def test_sampled_branch_raises_before_any_collective():
    w = world(2, False)
    with pytest.raises(NotImplementedError):
        _programs(w, rng=np.random.default_rng(0), candidate_samples=10)


def test_blocking_wrapper_runs_the_program():
    """evaluate_metrics_sharded with a one-rank world (no collective is issued) equals
    ttamm.evaluate_metrics on the same model."""
    w = world(2, False)

    class NoCollectives:
        def run(self, program):
            try:
                req = program.send(None)
            except StopIteration as stop:
                return stop.value
            raise AssertionError(f"world size 1 issued {req!r}")

    pairs = w.pairs
    got = evaluate_metrics_sharded(w.gm, RowOwnership(1, 0), comm=NoCollectives(), train_positive_map=w.prob.positives,
                                   val_interactions=pairs, item_feature_tensor=w.prob.item_features.cuda(),
                                   user_feature_tensor=w.prob.user_features.cuda(), num_items=w.shape.I, k_values=KS)
    want = ttamm.evaluate_metrics(w.gm, train_positive_map=w.prob.positives, val_interactions=pairs,
                                  item_feature_tensor=w.prob.item_features.cuda(),
                                  user_feature_tensor=w.prob.user_features.cuda(), device=torch.device("cuda"),
                                  num_items=w.shape.I, k_values=KS)
    assert got == want
