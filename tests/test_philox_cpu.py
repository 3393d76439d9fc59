"""oracle/philox.py, the CPU restatement of the drawn negative and dropout streams, checked on its
own: Random123's known answers for Philox4x32-10, the sampler's and the dropout stream's statistics,
that every input of a draw's counter and key reaches the output (what lets the device comparisons of
tests/test_rng_streams_gpu.py fail), and the keep thresholds.  Every seed is fixed: nothing here
can flake."""

from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import philox as px

SEED = 0x1234ABCD5678EF01


# ---------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _philox_scalar(c, k):
    """The round function transcribed on Python ints."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zero", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = px.philox4x32_10(*counter, *key)
    assert tuple(int(w) for w in got) == want
    assert _philox_scalar(counter, key) == want


def test_philox_vectorised_equals_scalar():
    """Broadcast counters (a column of keys against a row of groups) give each element's own draw."""
    rng = np.random.default_rng(5)
    c0 = rng.integers(0, 1 << 32, size=(7, 1), dtype=np.uint64)
    c1 = rng.integers(0, 1 << 32, size=(1, 5), dtype=np.uint64)
    got = px.philox4x32_10(c0, c1, 0xDEADBEEF, 0x2F00000F, 0x89ABCDEF, 0x01234567)
    for i in range(7):
        for j in range(5):
            want = _philox_scalar((int(c0[i, 0]), int(c1[0, j]), 0xDEADBEEF, 0x2F00000F), (0x89ABCDEF, 0x01234567))
            assert tuple(int(w[i, j]) for w in got) == want


def test_mulhi64_matches_python_ints():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 1 << 64, size=4096, dtype=np.uint64)
    a[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    for n in (2, 50, (1 << 31) + 7, (1 << 32) - 1, 1 << 32, (1 << 40) + 1, (1 << 64) - 1):
        want = [(int(x) * n) >> 64 for x in a]
        assert px.mulhi64(a, n).tolist() == want, n


# ---------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------
def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    val = np.array([x for v in lists for x in sorted(v)], dtype=np.int64)
    return off, val


def test_sampler_avoids_positives_unless_exhausted():
    """Lists on either side of the kernel's 32-entry register scan, a full-but-one list that exhausts,
    and users outside the CSR."""
    num_items = 64
    lists = [[], [7], list(range(31)), list(range(1, 33)), list(range(0, 66, 2)), list(range(45)),
             [i for i in range(64) if i != 17]]
    off, val = _csr(lists)
    users = np.arange(-2, 300, dtype=np.int64) % 9 - 1  # -1 .. 7: below and above the CSR's 7 rows too
    out, exhausted = px.negatives(users, 5, num_items, off, val, len(lists), SEED, 3, 12345)
    assert out.shape == exhausted.shape == (users.size, 5)
    assert out.min() >= 0 and out.max() < num_items
    for b, u in enumerate(users):
        pos = set(lists[u]) if 0 <= u < len(lists) else set()
        for j in range(5):
            assert (int(out[b, j]) in pos) == bool(exhausted[b, j]), (b, u, j)
    # only the 63-of-64 user can exhaust (the next fullest list rejects 45 / 64 per draw: 0.02 at 11 draws,
    # and an exhausted slot there would still be consistent above)
    assert exhausted[users == 6].mean() > 0.6  # (63 / 64)^11 = 0.84
    assert not exhausted[(users < 0) | (users >= len(lists))].any()
    # the accepted draw's index, stated a second way: 11 exactly where exhausted
    first = px.first_accepted_attempt(users, 5, num_items, off, val, len(lists), SEED, 3, 12345)
    assert np.array_equal(first == px.MAX_DRAWS, exhausted)
    for a in range(px.MAX_DRAWS):
        cand = px.negative_candidates(users.size * 5, num_items, SEED, 3, 12345, a).reshape(-1, 5)
        assert np.array_equal(out[first == a], cand[first == a].astype(np.int64))
    last = px.negative_candidates(users.size * 5, num_items, SEED, 3, 12345, px.MAX_DRAWS - 1).reshape(-1, 5)
    assert np.array_equal(out[exhausted], last[exhausted].astype(np.int64))  # the 11th candidate
    # a NULL CSR: nobody has positives
    free, ex = px.negatives(users, 5, num_items, None, None, 0, SEED, 3, 12345)
    first0 = px.negative_candidates(users.size * 5, num_items, SEED, 3, 12345, 0).reshape(-1, 5)
    assert not ex.any() and np.array_equal(free, first0.astype(np.int64))


def test_sampler_uniform_over_allowed_items():
    """tests/test_kernels_gpu.py::test_sampler_uniform_over_allowed_items on the restated stream."""
    num_items = 50
    blocked = list(range(0, 50, 5))
    off, val = _csr([blocked])
    out, exhausted = px.negatives(np.zeros(4000, dtype=np.int64), 10, num_items, off, val, 1, SEED, 0, 0)
    assert not exhausted.any()
    neg = out.reshape(-1)
    assert neg.size == 40000 and not np.isin(neg, blocked).any()
    counts = np.bincount(neg, minlength=num_items).astype(np.float64)
    allowed = [i for i in range(num_items) if i not in blocked]
    exp = neg.size / len(allowed)
    chi2 = float(((counts[allowed] - exp) ** 2 / exp).sum())
    print(f"chi2 = {chi2:.2f}")
    assert chi2 < 80.0  # 39 dof: p ~ 1e-4


# ---------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.15, 0.5])
def test_dropout_keep_rate_and_independence(p):
    rows, width = 4096, 256  # 2^20 decisions
    keep = px.dropout_keep(px.tower_row_keys(rows), width, p, SEED, 1, 0, 0).astype(np.float64)
    q = px.keep_threshold(p) / 65536.0

    def within(rate, n, want):
        # sigma of n Bernoulli(q) trials; a joint rate's own sigma sqrt(q^2 (1 - q^2) / n) where that is smaller
        sigma = math.sqrt(min(q * (1.0 - q), want * (1.0 - want)) / n)
        print(f"p={p}: rate {rate:.6f}, expected {want:.6f}, {abs(rate - want) / sigma:.2f} sigma over {n}")
        return abs(rate - want) <= 5.0 * sigma

    assert keep.size >= 1 << 20
    assert within(keep.mean(), keep.size, q)
    # two columns sharing a word (c, c + 1 with c even: its low and high halves)
    pair = keep[:, 0::2] * keep[:, 1::2]
    assert within(pair.mean(), pair.size, q * q)
    # one column in two adjacent rows
    adj = keep[:-1] * keep[1:]
    assert within(adj.mean(), adj.size, q * q)


BASE = dict(seed=SEED, counter=5, tower=0, layer=0)


@pytest.mark.parametrize("change", [dict(tower=1), dict(layer=1), dict(counter=6), dict(counter=(1 << 32) + 5),
                                    dict(seed=SEED ^ 1), dict(seed=SEED ^ (1 << 32))],
                         ids=["tower", "layer", "counter-lo", "counter-hi", "seed-lo", "seed-hi"])
def test_dropout_separation(change):
    keys = px.tower_row_keys(64)
    a = px.dropout_keep(keys, 40, 0.5, **BASE)
    b = px.dropout_keep(keys, 40, 0.5, **{**BASE, **change})
    # independent fair bits: 2560 decisions agree on 1280 +- 25; far from all
    assert 0.4 < (a != b).mean() < 0.6


def test_dropout_separation_row_key_and_columns():
    a = px.dropout_keep(np.array([3, 4, 3]), 40, 0.5, **BASE)
    assert np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])
    # the key is the row key's low word; the width only truncates
    assert np.array_equal(px.dropout_keep(np.array([3 + (1 << 32)]), 40, 0.5, **BASE)[0], a[0])
    assert np.array_equal(px.dropout_keep(np.array([3]), 12, 0.5, **BASE)[0], a[0, :12])
    # every column of a row is its own decision: no two of the 40 columns agree over 512 rows
    cols = px.dropout_keep(px.tower_row_keys(512), 40, 0.5, **BASE).T
    assert len({c.tobytes() for c in cols}) == 40
    # positive and negative item rows of the step hold distinct keys
    k = px.step_item_row_keys(32, 5)
    assert k.size == 192 and len(set(k.tolist())) == 192 and k[31] == 31 and k[32] == 32
    assert np.array_equal(px.step_user_row_keys(32), np.arange(32))


NEG_BASE = dict(seed=SEED, counter=5, slot_base=77)


@pytest.mark.parametrize("change", [dict(counter=6), dict(counter=(1 << 32) + 5), dict(seed=SEED ^ 1),
                                    dict(seed=SEED ^ (1 << 32)), dict(slot_base=78), dict(slot_base=(1 << 32) + 77)],
                         ids=["counter-lo", "counter-hi", "seed-lo", "seed-hi", "slot-base-lo", "slot-base-hi"])
def test_sampler_separation(change):
    users = np.zeros(200, dtype=np.int64)
    a, _ = px.negatives(users, 5, 1 << 20, None, None, 0, **NEG_BASE)
    b, _ = px.negatives(users, 5, 1 << 20, None, None, 0, **{**NEG_BASE, **change})
    assert (a != b).mean() > 0.99  # 2^20 items: two independent draws collide 1e-6 of the time
    if change == dict(slot_base=78):  # slot s of base 78 is slot s + 1 of base 77
        assert np.array_equal(a.reshape(-1)[1:], b.reshape(-1)[:-1])


def test_sampler_attempts_are_distinct_draws():
    c = [px.negative_candidates(1000, 1 << 20, SEED, 0, 0, a) for a in range(px.MAX_DRAWS)]
    for i in range(px.MAX_DRAWS):
        for j in range(i):
            assert (c[i] != c[j]).mean() > 0.99


# ---------------------------------------------------------------------------------------
# thresholds
# ---------------------------------------------------------------------------------------
def test_keep_thresholds():
    """float32(p) -> keep = 1f - p (one fp32 rounding) -> keep * 65536 (exact) -> truncation:
      p = 0      keep = 1                               65536, every 16-bit draw is below it: all kept
      p = 1e-5   keep = 0.99999 (fp32: 0.9999899864...)  * 65536 = 65535.34..  -> 65535
      p = 0.15   keep = 0.85 +- 6e-8                     * 65536 = 55705.6 +- 0.004 -> 55705
      p = 0.3    keep = 0.7 +- 6e-8                      * 65536 = 45875.2 +- 0.004 -> 45875
      p = 0.5    keep = 0.5                              32768
    (an fp32 rounding of keep moves the product by at most 2^-24 * 65536 = 0.004: no case is near an integer)."""
    assert px.keep_threshold(0.0) == 65536
    assert px.dropout_keep(px.tower_row_keys(64), 24, 0.0, SEED, 0, 0, 0).all()
    assert px.keep_threshold(1e-5) == 65535
    assert px.keep_threshold(0.15) == 55705
    assert px.keep_threshold(0.3) == 45875
    assert px.keep_threshold(0.5) == 32768
    # 65535: only the draw 0xFFFF is dropped
    h = px.dropout_halves(px.tower_row_keys(1024), 256, SEED, 0, 0, 0)
    assert np.array_equal(px.dropout_keep(px.tower_row_keys(1024), 256, 1e-5, SEED, 0, 0, 0), (h != 0xFFFF))
    assert h.dtype == np.uint32 and h.max() <= 0xFFFF
