"""On-device ranking metrics (csrc/metrics.hip, ttamm/metrics.py) against the oracle's restatement
of src/evaluation/metrics.py (oracle/cpu_reference.py: user_metrics, ranking_metrics).

Tolerances: recall / precision / hit_rate / mrr of one query are each ONE correctly rounded double
division of small integers, so they must be EQUAL.  ndcg and map are sums of at most 192 terms
<= 1, each a few ulp off (log2, a division), normalised to <= 1: worst case about 1e-13, so 1e-12
absolute; the means add n * 2^-53 relative from their fixed-order sum, still inside 1e-12."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import ttamm
from oracle import cpu_reference as ref
from ttamm import _lib

pytestmark = pytest.mark.gpu

NAMES = ("recall", "precision", "ndcg", "hit_rate", "map")
EXACT = ("recall", "precision", "hit_rate")
TOL = 1e-12


def _raw(pred, toff, tval, ks, *, pad=False, per_user=True):
    """ttamm_ranking_metrics through ctypes: (summary [5 n_k + 2], rows [nq, 5 n_k + 1]) as numpy."""
    lib = _lib.load()
    dev = torch.device("cuda")
    pred, toff, tval = pred.to(dev), toff.to(dev), tval.to(dev)
    nq, k_pred = pred.shape
    ncol = 5 * len(ks) + 1
    summary = torch.full((ncol + 1,), -7.0, dtype=torch.float64, device=dev)
    rows = torch.full((nq, ncol), -7.0, dtype=torch.float64, device=dev) if per_user else None
    ws_bytes = lib.ttamm_ranking_metrics_workspace_size(nq, len(ks))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_ranking_metrics(
        pred.data_ptr() if pred.numel() else None, nq, k_pred, max(pred.stride(0), k_pred), toff.data_ptr(),
        tval.data_ptr() if tval.numel() else None, (ctypes.c_int32 * len(ks))(*ks), len(ks), 1 if pad else 0,
        rows.data_ptr() if per_user else None, ncol, summary.data_ptr(), ws.data_ptr(), ws_bytes,
        _lib.stream_handle(dev)))
    torch.cuda.synchronize()
    return summary.cpu().numpy(), (rows.cpu().numpy() if per_user else None)


def _csr(truths):
    toff = np.zeros(len(truths) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in truths], out=toff[1:])
    tval = np.fromiter((i for t in truths for i in sorted(t)), dtype=np.int64)
    return torch.from_numpy(toff), torch.from_numpy(tval)


def _check_against_oracle(lists, truths, ks, summary, rows):
    """lists[q]: the list the reference would see for query q (holes dropped, padding applied)."""
    counted = 0
    for q, (lst, truth) in enumerate(zip(lists, truths)):
        if not truth:
            assert not rows[q].any(), q  # not counted: an all-zero row
            continue
        counted += 1
        want = ref.user_metrics(lst, truth, ks)
        for j, k in enumerate(ks):
            for m, name in enumerate(NAMES):
                got, exp = rows[q, 5 * j + m], want[f"{name}@{k}"]
                if name in EXACT:
                    assert got == exp, (q, name, k, got, exp, lst, sorted(truth)[:8])
                else:
                    assert abs(got - exp) <= TOL, (q, name, k, got, exp)
        assert rows[q, 5 * len(ks)] == want["mrr"], (q, rows[q, 5 * len(ks)], want["mrr"])
    means = ref.ranking_metrics({q: l for q, l in enumerate(lists)}, {q: t for q, t in enumerate(truths)}, ks)
    for j, k in enumerate(ks):
        for m, name in enumerate(NAMES):
            assert abs(summary[5 * j + m] - getattr(means, name)[k]) <= TOL, (name, k)
    assert abs(summary[5 * len(ks)] - means.mrr) <= TOL
    assert summary[5 * len(ks) + 1] == counted


def _random_rows(nq, k_pred, max_k, seed):
    """Rows and truth sets cycling through 8 row kinds x 5 truth sizes (8 and 5 are coprime, so
    every pair occurs within 40 queries)."""
    rng = np.random.default_rng(seed)
    universe = 1000
    sizes = [0, 1, 2, max_k, 300]
    rows = np.full((nq, k_pred), -1, dtype=np.int64)
    truths = []
    for q in range(nq):
        T = sizes[q % 5]
        truth = set(rng.choice(universe, size=T, replace=False).tolist())
        others = np.setdiff1d(np.arange(universe), np.fromiter(truth, dtype=np.int64, count=len(truth)))
        tl = sorted(truth)
        kind = q % 8
        if kind == 0:  # all hits (as far as the truth reaches; cycled, so ids repeat when T < k_pred)
            row = [tl[i % T] for i in range(k_pred)] if T else rng.choice(others, size=k_pred).tolist()
        elif kind == 1:  # no hit
            row = rng.choice(others, size=k_pred, replace=False).tolist()
        else:
            miss = rng.choice(others, size=k_pred)
            row = np.where(rng.random(k_pred) < 0.3, rng.choice(tl, size=k_pred) if T else miss, miss).tolist()
            if kind == 2:  # holes at the tail
                row[k_pred - (k_pred + 2) // 3:] = [-1] * ((k_pred + 2) // 3)
            elif kind == 3:  # holes in the middle (and at the head)
                for p in range(0, k_pred, 3):
                    row[p] = -1
            elif kind == 4:  # only holes
                row = [-1] * k_pred
            elif kind == 5 and T:  # a repeated id that is in the truth
                for p in range(0, k_pred, 2):
                    row[p] = tl[0]
            elif kind == 6:  # a repeated id that is not in the truth
                for p in range(0, k_pred, 2):
                    row[p] = int(others[0])
        rows[q] = row
        truths.append(truth)
    return rows, truths


@pytest.mark.parametrize("ks", [[20, 5, 10], [1], [192], [3, 64, 65, 128, 129, 192]], ids=lambda k: "k" + "_".join(map(str, k)))
@pytest.mark.parametrize("k_pred", [1, 7, 64, 65, 192])
def test_kernel_matches_oracle_on_random_rows(k_pred, ks):
    nq = 257
    rows, truths = _random_rows(nq, k_pred, max(ks), seed=1000 * k_pred + len(ks))
    toff, tval = _csr(truths)
    summary, got = _raw(torch.from_numpy(rows), toff, tval, ks)
    lists = [[i for i in r if i >= 0] for r in rows.tolist()]
    _check_against_oracle(lists, truths, ks, summary, got)
    # the tensor API: same numbers, the counted queries' rows in order
    m = ttamm.ranking_metrics(torch.from_numpy(rows).cuda(), toff.cuda(), tval.cuda(), ks, per_user=True)
    assert len(m.per_user) == sum(1 for t in truths if t)
    for j, k in enumerate(ks):
        for i, name in enumerate(NAMES):
            assert getattr(m, name)[k] == summary[5 * j + i]
    assert m.mrr == summary[5 * len(ks)]
    first = next(q for q, t in enumerate(truths) if t)
    assert m.per_user[0] == {**{f"{name}@{k}": got[first, 5 * j + i] for j, k in enumerate(ks)
                                for i, name in enumerate(NAMES)}, "mrr": got[first, 5 * len(ks)]}


def test_without_per_user_rows_the_summary_is_the_same():
    rows, truths = _random_rows(257, 20, 20, seed=5)
    toff, tval = _csr(truths)
    with_rows, _ = _raw(torch.from_numpy(rows), toff, tval, [5, 10, 20])
    without, none = _raw(torch.from_numpy(rows), toff, tval, [5, 10, 20], per_user=False)
    assert none is None and np.array_equal(with_rows, without)


def test_strided_rows_and_empty_shapes():
    """ld_pred wider than k_pred is respected; no queries / no columns give zeros."""
    rows, truths = _random_rows(70, 20, 10, seed=6)
    toff, tval = _csr(truths)
    wide = torch.full((70, 33), 5, dtype=torch.long)  # 5 may be anyone's truth: must not be read
    wide[:, :20] = torch.from_numpy(rows)
    a, ra = _raw(torch.from_numpy(rows), toff, tval, [10])
    b, rb = _raw(wide.cuda()[:, :20], toff, tval, [10])
    assert np.array_equal(a, b) and np.array_equal(ra, rb)
    s, _ = _raw(torch.zeros((0, 20), dtype=torch.long), torch.zeros(1, dtype=torch.long),
                torch.zeros(0, dtype=torch.long), [5, 10], per_user=False)
    assert not s.any()
    s, r = _raw(torch.zeros((70, 0), dtype=torch.long), toff, tval, [10])
    assert not r.any() and not s[:-1].any() and s[-1] == sum(1 for t in truths if t)
    with pytest.raises(ValueError, match="non-decreasing"):
        ttamm.ranking_metrics(torch.from_numpy(rows).cuda(), torch.flip(toff, [0]).cuda(), tval.cuda(), [10])


@pytest.mark.parametrize("k_pred,ks", [(20, [5, 10, 20]), (7, [20, 5]), (64, [65, 3])])
def test_pad_with_truth_follows_the_reference_rule(k_pred, ks):
    """training.py:969-972 restated: (valid + [t for t in truth if t not in valid])[:max_k]."""
    max_k = max(ks)
    rng = np.random.default_rng(k_pred)
    universe = 400
    rows, truths = [], []
    valid_counts = [0, 1, max_k - 1, max_k, k_pred, k_pred // 2]
    truth_sizes = [1, 3, max_k, 2 * max_k + 5]
    for nv in valid_counts:
        nv = min(nv, k_pred)
        for T in truth_sizes:
            for listed in (0, 1, 2):  # how much of the truth the valid ids already hold
                truth = sorted(rng.choice(universe, size=T, replace=False).tolist())
                others = np.setdiff1d(np.arange(universe), truth)
                take = min(nv, T) if listed == 2 else min(nv, T, listed)
                valid = list(rng.permutation(np.concatenate([
                    rng.choice(truth, size=take, replace=False), rng.choice(others, size=nv - take, replace=False)]
                ).astype(np.int64)))
                row = np.full(k_pred, -1, dtype=np.int64)
                where = np.sort(rng.choice(k_pred, size=nv, replace=False))  # holes anywhere
                row[where] = valid
                rows.append(row)
                truths.append(set(truth))
    # a repeated relevant id in a short list: the id is listed, so it is not appended again
    row = np.full(k_pred, -1, dtype=np.int64)
    row[: min(3, k_pred)] = 11
    rows.append(row)
    truths.append({11, 12, 13})
    rows = np.stack(rows)
    toff, tval = _csr(truths)
    summary, got = _raw(torch.from_numpy(rows), toff, tval, ks, pad=True)
    lists = []
    for r, truth in zip(rows.tolist(), truths):
        valid = [i for i in r if i >= 0]
        if len(valid) < max_k:
            valid = (valid + [t for t in truth if t not in valid])[:max_k]
        lists.append(valid)
    assert any(len(l) < max_k for l in lists) and any(len(l) == max_k for l in lists)
    _check_against_oracle(lists, truths, ks, summary, got)


def test_bit_identical_runs_and_a_grid_past_65535():
    nq, k_pred, ks = 70_000, 20, [5, 10, 20]
    g = torch.Generator().manual_seed(3)
    pred = torch.randint(-1, 50, (nq, k_pred), generator=g)
    member = torch.rand((nq, 50), generator=g) < 0.04  # 0 .. about 6 truth items, ascending and unique
    toff = torch.zeros(nq + 1, dtype=torch.long)
    toff[1:] = member.sum(dim=1).cumsum(0)
    tval = member.nonzero()[:, 1].contiguous()
    s1, r1 = _raw(pred, toff, tval, ks)
    s2, r2 = _raw(pred, toff, tval, ks)
    assert np.array_equal(s1, s2) and np.array_equal(r1, r2)
    counted = (toff[1:] > toff[:-1]).numpy()
    assert s1[-1] == counted.sum() and 0 < counted.sum() < nq
    assert not r1[~counted].any()
    assert np.abs(s1[:-1] - r1[counted].mean(axis=0, dtype=np.float64)).max() <= TOL
    assert 0.0 < s1[0] < 1.0  # hits and misses both occur
    # a few rows against the oracle, the last one included
    for q in [0, 1, 65_535, 65_536, nq - 1]:
        if counted[q]:
            want = ref.user_metrics([i for i in pred[q].tolist() if i >= 0],
                                    set(tval[toff[q]:toff[q + 1]].tolist()), ks)
            assert r1[q, 0] == want["recall@5"] and abs(r1[q, 12] - want["ndcg@20"]) <= TOL


def test_dict_api_matches_the_oracle():
    rng = np.random.default_rng(17)
    ks = [10, 3, 20]
    preds, truth = {}, {}
    for u in rng.permutation(60).tolist():  # users in no particular order
        n = int(rng.integers(0, 30))
        preds[u] = rng.integers(0, 40, size=n).tolist()
        truth[u] = set(rng.integers(0, 40, size=int(rng.integers(1, 6))).tolist())
    preds[100] = [1, 2, 3]          # in the predictions, absent from the truth
    truth[7] = set()                # present with an empty set
    truth[200] = {1}                # in the truth, absent from the predictions
    preds[101] = list(range(250))   # longer than 192: cut to max(k_values)
    truth[101] = {5, 19, 230}
    preds[102] = [-4, 5, -4, 9]     # the reference compares any integers: negative ids are not holes
    truth[102] = {-4, 9}
    got = ttamm.compute_ranking_metrics(preds, truth, ks)
    want = ref.ranking_metrics(preds, truth, ks)
    for name in NAMES:
        assert list(getattr(got, name)) == ks
        for k in ks:
            assert abs(getattr(got, name)[k] - getattr(want, name)[k]) <= TOL, (name, k)
    assert abs(got.mrr - want.mrr) <= TOL
    order = [u for u in preds if truth.get(u)]
    assert len(got.per_user) == len(order)
    for u, row in zip(order, got.per_user):
        exp = ref.user_metrics(preds[u], truth[u], ks)
        assert set(row) == set(exp)
        for key, v in exp.items():
            if key.split("@")[0] in EXACT or key == "mrr":
                assert row[key] == v, (u, key)
            else:
                assert abs(row[key] - v) <= TOL, (u, key)
    assert ttamm.compute_ranking_metrics(preds, truth, ks, per_user=False).per_user == []


# ---------------------------------------------------------------------------------------
# evaluate_metrics == compute_ranking_metrics(*evaluate_model(...))
# ---------------------------------------------------------------------------------------
KS = [5, 10, 20]


@pytest.fixture(scope="module")
def trained():
    """A tiny trained model with 30 items, about 11 of them blocked per user: fewer than
    max_k = 20 remain for most users, so the padding path runs end to end."""
    from gpu_helpers import run_ttamm
    from helpers import Shape, make_problem

    shape = Shape(U=48, I=30, B=32)
    prob = make_problem(shape, seed=21, steps=2, positives_per_user=14)
    model, _, _ = run_ttamm(prob, steps=2)
    model.eval()
    rng = np.random.default_rng(4)
    val = []
    for u in rng.permutation(shape.U).tolist():
        if u % 11 == 0:
            continue  # users without validation pairs
        items = rng.integers(0, shape.I, size=int(rng.integers(1, 4))).tolist()
        val += [(u, i) for i in items]
    val += val[:7]  # duplicate pairs
    val = [val[i] for i in rng.permutation(len(val)).tolist()]
    return prob, model, val


def _args(prob, model, **kw):
    dev = torch.device("cuda")
    base = dict(train_positive_map=prob.positives, item_feature_tensor=prob.item_features.to(dev),
                user_feature_tensor=prob.user_features.to(dev), device=dev, num_items=prob.shape.I, k_values=KS)
    base.update(kw)
    return base


def _assert_same(got, want):
    for name in NAMES:
        for k in KS:
            assert abs(getattr(got, name)[k] - getattr(want, name)[k]) <= TOL, (name, k, getattr(got, name), getattr(want, name))
    assert abs(got.mrr - want.mrr) <= TOL


def _branch(prob, model, branch):
    """(model, extra keyword arguments as a factory: rngs must be fresh for every call)."""
    from torch import nn

    if branch == "dot":
        return lambda: {}
    if branch == "cosine":
        model.similarity = nn.CosineSimilarity(dim=-1)
        return lambda: {}
    if branch == "faiss":
        model.similarity = nn.CosineSimilarity(dim=-1)
        res = ttamm.prepare_faiss_resources(model, num_items=prob.shape.I, item_features=prob.item_features.cuda(),
                                            device=torch.device("cuda"))
        assert res["normalize"]
        return lambda: {"faiss_resources": res}
    assert branch == "sampled"
    return lambda: {"rng": np.random.default_rng(99), "candidate_samples": 12}


@pytest.mark.parametrize("branch", ["dot", "cosine", "faiss", "sampled"])
def test_evaluate_metrics_equals_metrics_of_evaluate_model(trained, branch):
    prob, model, val = trained
    similarity = model.similarity
    try:
        extra = _branch(prob, model, branch)
        preds, truth = ttamm.evaluate_model(model, val_interactions=val, **_args(prob, model, **extra()))
        assert len(truth) == len({u for u, _ in val})
        if branch != "sampled":  # short lists were padded with the truth
            assert any(len(set(range(prob.shape.I)) - prob.positives[u]) < max(KS) for u in truth)
        want = ref.ranking_metrics(preds, truth, KS)
        assert want.recall[20] > 0.0
        csr = ttamm.PositivesCSR.from_mapping(prob.positives, device=torch.device("cuda"))
        val_t = torch.tensor(val, dtype=torch.long, device="cuda")
        for v in (val, val_t):
            for positives in (prob.positives, csr):
                got = ttamm.evaluate_metrics(model, val_interactions=v,
                                             **_args(prob, model, train_positive_map=positives, **extra()))
                _assert_same(got, want)
                assert got.per_user == []
        got = ttamm.evaluate_metrics(model, val_interactions=val_t, per_user=True,
                                     **_args(prob, model, train_positive_map=csr, **extra()))
        _assert_same(got, want)
        users = sorted(truth)  # groupby order
        assert len(got.per_user) == len(users)
        for u, row in zip(users, got.per_user):
            exp = ref.user_metrics(preds[u], truth[u], KS)
            assert row["recall@20"] == exp["recall@20"] and row["mrr"] == exp["mrr"], u
            assert abs(row["ndcg@10"] - exp["ndcg@10"]) <= TOL
    finally:
        model.similarity = similarity


def test_evaluate_metrics_takes_a_dataframe(trained):
    pd = pytest.importorskip("pandas")
    prob, model, val = trained
    df = pd.DataFrame(val, columns=["user_idx", "item_idx"])
    preds, truth = ttamm.evaluate_model(model, val_interactions=df, **_args(prob, model))
    want = ref.ranking_metrics(preds, truth, KS)
    _assert_same(ttamm.evaluate_metrics(model, val_interactions=df, **_args(prob, model)), want)
    kw = lambda: {"rng": np.random.default_rng(5), "candidate_samples": 8}  # noqa: E731
    preds, truth = ttamm.evaluate_model(model, val_interactions=df, **_args(prob, model, **kw()))
    want = ref.ranking_metrics(preds, truth, KS)
    _assert_same(ttamm.evaluate_metrics(model, val_interactions=df, **_args(prob, model, **kw())), want)


def test_evaluate_metrics_without_pairs_is_all_zero(trained):
    prob, model, _ = trained
    got = ttamm.evaluate_metrics(model, val_interactions=[], **_args(prob, model))
    assert got.recall == {k: 0.0 for k in KS} and got.mrr == 0.0 and got.per_user == []
