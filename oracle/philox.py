"""CPU restatement of ttamm's two on-device random streams: the negative sampler
(csrc/sampler.hip sample_slot) and the dropout keep decisions drawn in the GEMM epilogues
(csrc/gemm.hip epilogue_hidden_pair / epilogue8_hidden, keyed by csrc/tower.hip set_dropout).

TEST INFRASTRUCTURE ONLY: tests/ use it as the checker of the HIP kernels; the product never
imports it.

Both streams are Philox4x32-10 (Salmon et al., SC'11; csrc/common.h philox4x32) on counters that
name the decision, so every draw is a pure function of (seed, step counter, position):

    negatives, slot s = b * num_neg + j, key = slot_base + s, draw `attempt` in 0..10:
        philox(c = (key lo, key hi, counter lo, 1 << 28 | attempt << 20 | (counter >> 32) & 0xFFFFF),
               k = (seed lo, seed hi)) -> (x, y, ., .)
        candidate = (((x << 32) | y) * num_items) >> 64
        the first candidate that is not one of user b's positives is written; after 11 rejected
        draws the 11th candidate is written and the slot counts as exhausted

    dropout, column c of a row with key k, tower t (0 user, 1 item), hidden layer l:
        philox(c = (k & 0xFFFFFFFF, c >> 3, counter lo, 2 << 28 | t << 24 | l << 20 | (counter >> 32) & 0xFFFFF),
               k = (seed lo, seed hi)) -> 4 words
        u = the (c odd ? high : low) 16 bits of word (c & 7) >> 1
        keep iff u < min(65536, int(float32(1 - p) * 65536))

Everything is integer arithmetic on numpy uint64 arrays masked to 32 bits, vectorised over slots /
rows x column groups; parity with the device is bit-exact."""

from __future__ import annotations

import numpy as np

M32 = (1 << 32) - 1
_U = np.uint64
_M32 = _U(M32)
_S32 = _U(32)

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85

RNG_NEGATIVES = 1 << 28
RNG_DROPOUT = 2 << 28
MAX_DRAWS = 11


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counter (c0, c1, c2, c3) and key (k0, k1): four uint64 arrays holding the
    32-bit output words (inputs broadcast against each other; only their low 32 bits count)."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=_U) & _M32 for v in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & M32, int(k1) & M32
    m0, m1 = _U(PHILOX_M0), _U(PHILOX_M1)
    for _ in range(10):
        p0 = c0 * m0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = c2 * m1
        hi0, lo0 = p0 >> _S32, p0 & _M32
        hi1, lo1 = p1 >> _S32, p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ _U(k0), lo1, hi0 ^ c3 ^ _U(k1), lo0
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def mulhi64(a: np.ndarray, n: int) -> np.ndarray:
    """(a * n) >> 64 for a uint64 array a and 0 <= n < 2^64, by 32-bit limbs."""
    a = np.asarray(a, dtype=_U)
    n = int(n)
    assert 0 <= n < (1 << 64)
    nl, nh = _U(n & M32), _U(n >> 32)
    ah, al = a >> _S32, a & _M32
    t = al * nl
    t = ah * nl + (t >> _S32)
    w1, w2 = t & _M32, t >> _S32
    t = al * nh + w1
    return ah * nh + w2 + (t >> _S32)


def _words(v: int) -> tuple[int, int]:
    v = int(v) & ((1 << 64) - 1)
    return v & M32, v >> 32


def negative_candidates(slots: int, num_items: int, seed: int, counter: int, slot_base: int, attempt: int) -> np.ndarray:
    """Draw `attempt` of slots 0..slots-1: the candidate item of each, uint64 [slots]."""
    key = (np.arange(slots, dtype=_U) + _U(int(slot_base) & ((1 << 64) - 1)))  # wraps as int64 addition does
    clo, chi = _words(counter)
    k0, k1 = _words(seed)
    c3 = RNG_NEGATIVES | (int(attempt) << 20) | (chi & 0xFFFFF)
    x, y, _, _ = philox4x32_10(key & _M32, key >> _S32, clo, c3, k0, k1)
    return mulhi64((x << _S32) | y, num_items)


def negatives(users, num_neg: int, num_items: int, pos_offsets, pos_values, user_rows: int, seed: int, counter: int,
              slot_base: int):
    """ttamm_sample_negatives: (out int64 [batch, num_neg], exhausted bool [batch, num_neg]).
    pos_offsets None (a NULL CSR), or a user id outside [0, user_rows): no positives."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    batch = users.shape[0]
    slots = batch * int(num_neg)
    u = np.repeat(users, num_neg)
    if pos_offsets is None:
        known = np.zeros(slots, dtype=bool)
        pos_keys = np.zeros(0, dtype=np.int64)
        stride = 1
    else:
        off = np.asarray(pos_offsets, dtype=np.int64)
        val = np.asarray(pos_values, dtype=np.int64)
        known = (u >= 0) & (u < user_rows)
        deg = off[1:user_rows + 1] - off[:user_rows]
        used = val[off[0]:off[user_rows]] if user_rows > 0 else val[:0]
        stride = int(used.max()) + 1 if used.size else 1
        assert used.size == 0 or int(used.min()) >= 0
        assert (user_rows + 1) * stride < (1 << 62)
        # one sorted-free membership set of (user, item) pairs: user * stride + item
        pos_keys = np.repeat(np.arange(user_rows, dtype=np.int64), deg) * stride + used
    out = np.zeros(slots, dtype=np.int64)
    open_ = np.ones(slots, dtype=bool)  # no accepted draw yet
    for attempt in range(MAX_DRAWS):
        cand = negative_candidates(slots, num_items, seed, counter, slot_base, attempt).astype(np.int64)
        out[open_] = cand[open_]
        small = known & (cand < stride)
        hit = np.zeros(slots, dtype=bool)
        if pos_keys.size:
            hit[small] = np.isin(u[small] * stride + cand[small], pos_keys)
        open_ &= hit
    return out.reshape(batch, num_neg), open_.reshape(batch, num_neg)


def first_accepted_attempt(users, num_neg: int, num_items: int, pos_offsets, pos_values, user_rows: int, seed: int,
                           counter: int, slot_base: int) -> np.ndarray:
    """The index (0..10) of the draw each slot accepted, 11 for an exhausted slot; int64 [batch, num_neg].
    (A second statement of the retry chain, attempt by attempt on truncated chains.)"""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    pos = {}
    if pos_offsets is not None:
        off = np.asarray(pos_offsets, dtype=np.int64)
        val = np.asarray(pos_values, dtype=np.int64)
        for b in set(users.tolist()):
            if 0 <= b < user_rows:
                pos[b] = val[off[b]:off[b + 1]]
    slots = users.shape[0] * int(num_neg)
    u = np.repeat(users, num_neg)
    first = np.full(slots, MAX_DRAWS, dtype=np.int64)
    for attempt in reversed(range(MAX_DRAWS)):
        cand = negative_candidates(slots, num_items, seed, counter, slot_base, attempt).astype(np.int64)
        ok = np.ones(slots, dtype=bool)
        for b, items in pos.items():
            sel = u == b
            ok[sel] = ~np.isin(cand[sel], items)
        first[ok] = attempt
    return first.reshape(users.shape[0], num_neg)


def keep_threshold(p: float) -> int:
    """min(65536, int(float32(float32(1) - float32(p)) * 65536)) (gemm.hip keep_threshold16 of
    tower.hip set_dropout's keep_prob)."""
    keep = np.float32(1.0) - np.float32(p)
    t = np.float32(keep * np.float32(65536.0))  # exact: a power-of-two scale
    return 65536 if t >= np.float32(65536.0) else int(t)


def dropout_halves(row_keys, width: int, seed: int, counter: int, tower: int, layer: int) -> np.ndarray:
    """The 16-bit uniform of every (row, column): uint32 [rows, width]."""
    keys = np.asarray(row_keys, dtype=np.int64).reshape(-1).astype(_U) & _M32
    groups = (int(width) + 7) // 8
    clo, chi = _words(counter)
    k0, k1 = _words(seed)
    c3 = RNG_DROPOUT | (int(tower) << 24) | (int(layer) << 20) | (chi & 0xFFFFF)
    w = philox4x32_10(keys[:, None], np.arange(groups, dtype=_U)[None, :], clo, c3, k0, k1)
    words = np.stack(w, axis=-1)  # [rows, groups, 4]
    halves = np.stack([words & _U(0xFFFF), (words >> _U(16)) & _U(0xFFFF)], axis=-1)  # [..., 4, (low, high)]
    return halves.reshape(keys.shape[0], groups * 8)[:, :width].astype(np.uint32)


def dropout_keep(row_keys, width: int, p: float, seed: int, counter: int, tower: int, layer: int) -> np.ndarray:
    """The keep mask of one hidden layer: uint8 [rows, width], 1 = kept."""
    return (dropout_halves(row_keys, width, seed, counter, tower, layer) < keep_threshold(p)).astype(np.uint8)


# ---- row keys of the three callers ------------------------------------------------------------
TOWER_USER, TOWER_ITEM = 0, 1


def tower_row_keys(n: int) -> np.ndarray:
    """ttamm_tower_train_forward: row r has key r (and draws as tower 0)."""
    return np.arange(n, dtype=np.int64)


def step_user_row_keys(batch: int, row_base: int = 0) -> np.ndarray:
    """The step's user rows (tower 0): row_base + r; row_base is 0 in one process."""
    return row_base + np.arange(batch, dtype=np.int64)


def step_item_row_keys(batch: int, num_neg: int) -> np.ndarray:
    """The one-process step's item rows (tower 1): row r < B (interaction r's positive) has key r,
    row r >= B (negative slot r - B) has key B + (r - B)."""
    r = np.arange(batch * (1 + num_neg), dtype=np.int64)
    return np.where(r < batch, r, batch + (r - batch))
