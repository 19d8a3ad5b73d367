"""GPU: csm_list_select -- the device selection the reduced finish of
csm_search_match runs over a collected list (csrc/csm_select.hip: radix select
of the K-th largest key, then a compaction) -- against the definition restated
in numpy:

  S = { h : pred(h) and (key(h) >= key_K or (band_on and DoubleEqual(h.score, best, 1e-2))) }

key: the order-preserving 64-bit image of score + 0.0; key_K: the K-th largest
key among the hits passing pred (the lowest when fewer than K pass); pred:
always, or the angular list's near-best test on the candidate's (x, y).
Every comparison is exact: the sets are equal, the scores bit-equal, n_out the
full count."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGN = np.uint64(1) << np.uint64(63)


def key(score):
    s = np.asarray(score, dtype=np.float64) + 0.0  # -0.0 -> +0.0
    u = s.view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | SIGN)


def within_tol(d, tol):  # util::DoubleEqual on d = a - b
    return np.where(d < 0.0, d >= -abs(tol), d <= abs(tol))


def near_pred(flat, near):
    x0, y0, step, ns, bx, by, tol = near
    ns = int(ns)
    x = x0 + ((flat // ns) % ns) * step
    y = y0 + (flat % ns) * step
    return within_tol(x - bx, tol) & within_tol(y - by, tol)


def ref_select(score, flat, k, band_on=False, best=0.0, near=None):
    """Indices into the list of the members of S, ascending flat."""
    score = np.asarray(score, dtype=np.float64)
    flat = np.asarray(flat, dtype=np.int64)
    pred = np.ones(score.size, dtype=bool) if near is None else near_pred(flat, near)
    ks = key(score)
    passing = np.sort(ks[pred])[::-1]
    key_k = passing[min(k, passing.size) - 1] if passing.size else np.uint64(0)
    member = pred & ((ks >= key_k) | (within_tol(score - best, 1e-2) if band_on else False))
    idx = np.nonzero(member)[0]
    return idx[np.argsort(flat[idx], kind="stable")]


@pytest.fixture(scope="module")
def ctx():
    import roborts_csm
    c = roborts_csm.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(ctx, score, flat, k, band_on=False, best=0.0, near=None):
    score = np.asarray(score, dtype=np.float64)
    flat = np.asarray(flat, dtype=np.int64)
    want = ref_select(score, flat, k, band_on, best, near)
    got_flat, got_score, n = ctx.list_select(score, flat, k, band_on, best, near)
    assert n == want.size, (n, want.size)
    assert np.array_equal(got_flat[:n], flat[want])
    assert same_bits(got_score[:n], score[want])
    return n


def shuffled_flat(rng, n, span=None):
    return rng.permutation(span or n)[:n].astype(np.int64)


# 256 * 2048 + 1: one hit past a full grid of 2048 blocks of 256 (the grid-stride tail)
SIZES = [1, 21, 22, 23, 64, 65, 70001, 256 * 2048 + 1]


@pytest.mark.parametrize("k", [22, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_distinct_scores(ctx, n, k):
    rng = np.random.default_rng(1000 + n + k)
    score = rng.permutation(n) / float(n) - 0.25  # distinct, both signs
    assert check(ctx, score, shuffled_flat(rng, n), k) == min(n, k)


@pytest.mark.parametrize("k", [22, 1])
@pytest.mark.parametrize("n", [23, 65, 70001])
def test_sizes_random_scores_with_ties(ctx, n, k):
    rng = np.random.default_rng(2000 + n + k)
    score = rng.integers(0, max(3, n // 7), n) / 64.0  # many equal scores
    assert check(ctx, score, shuffled_flat(rng, n), k) >= min(n, k)


def test_capacity_counts_and_stops(ctx):
    """A capacity of 7 under a selection of 22: the count is exact, the seven
    written are members, nothing is written past them."""
    import roborts_csm
    from roborts_csm import _lib
    rng = np.random.default_rng(7)
    n, k, cap = 300, 22, 7
    score = rng.permutation(n) / float(n)
    flat = shuffled_flat(rng, n)
    want = ref_select(score, flat, k)
    assert want.size == 22
    out_flat = np.full(cap + 16, -5, dtype=np.int64)
    out_score = np.full(cap + 16, -5.0)
    n_out = C.c_int64(-1)
    near = np.zeros(7)
    ctx._check(_lib.csm_list_select(ctx._h, roborts_csm._dptr(score), roborts_csm._i64ptr(flat), n, k, 0, 0.0, 0,
                                    roborts_csm._dptr(near), roborts_csm._i64ptr(out_flat),
                                    roborts_csm._dptr(out_score), cap, C.byref(n_out)))
    assert n_out.value == 22
    assert (out_flat[cap:] == -5).all() and (out_score[cap:] == -5.0).all()
    assert np.isin(out_flat[:cap], flat[want]).all() and np.unique(out_flat[:cap]).size == cap
    assert (np.diff(out_flat[:cap]) > 0).all()
    by_flat = dict(zip(flat.tolist(), score.tolist()))
    assert same_bits(out_score[:cap], [by_flat[f] for f in out_flat[:cap].tolist()])


def test_keys_differ_only_in_the_lowest_digit(ctx):
    rng = np.random.default_rng(11)
    n = 3000
    u = np.float64(0.8125).view(np.uint64) + rng.integers(0, 512, n).astype(np.uint64)  # the key's last 9 bits
    score = u.view(np.float64)
    assert np.unique(key(score) >> np.uint64(9)).size == 1
    for k in (22, 1):
        check(ctx, score, shuffled_flat(rng, n), k)


def test_keys_differ_only_in_the_highest_digit(ctx):
    rng = np.random.default_rng(12)
    e = rng.integers(-120, 120, 900)
    score = np.where(rng.random(900) < 0.5, -1.0, 1.0) * 4.0 ** e  # sign and exponent: the key's top 11 bits
    assert np.unique(key(score) & np.uint64((1 << 53) - 1)).size <= 2  # all zeros, or all ones below a negative's digit
    for k in (22, 1):
        check(ctx, score, shuffled_flat(rng, score.size), k)


@pytest.mark.parametrize("n", [1, 22, 23, 5000])
def test_all_scores_equal(ctx, n):
    rng = np.random.default_rng(13)
    assert check(ctx, np.full(n, 0.625), shuffled_flat(rng, n), 22) == n  # closed under ties with the K-th


@pytest.mark.parametrize("copies", [21, 22, 23])
def test_copies_of_the_top_value_around_k(ctx, copies):
    """K - 1, K and K + 1 copies of the top value: the K-th is the next value
    below, the top itself, and the top with one more tied member."""
    rng = np.random.default_rng(14 + copies)
    n, k = 400, 22
    score = rng.permutation(n) / (2.0 * n)
    score[rng.permutation(n)[:copies]] = 0.75
    assert check(ctx, score, shuffled_flat(rng, n), k) == max(k, copies)


def test_negative_zero_and_positive_scores(ctx):
    rng = np.random.default_rng(15)
    n = 600
    score = rng.permutation(n) / float(n) - 0.97  # a few positive, most negative
    score[rng.permutation(n)[:40]] = np.where(np.arange(40) % 2 == 0, 0.0, -0.0)
    flat = shuffled_flat(rng, n)
    pos, nz = int((score > 0).sum()), int((score == 0.0).sum())
    assert 0 < pos < 22 and nz >= 40 and np.signbit(score[score == 0.0]).any() and not np.signbit(score[score == 0.0]).all()
    # K lands among the zeros: -0.0 and +0.0 share a key, all of them come along
    assert check(ctx, score, flat, 22) == pos + nz
    assert check(ctx, score, flat, pos) == pos
    assert check(ctx, score, flat, pos + nz + 1) == pos + nz + 1  # ... and past them, into the negatives
    assert check(ctx, -np.abs(score) - 0.5, flat, 22) >= 22  # all negative


@pytest.mark.parametrize("band", [5, 22, 300, 12000])
def test_band_shorter_and_longer_than_k(ctx, band):
    rng = np.random.default_rng(16 + band)
    n = 20000
    best = 0.875
    score = rng.permutation(n) / float(n) * 0.8  # distinct, below the band
    inb = rng.permutation(n)[:band]
    score[inb] = best - 0.01 * rng.permutation(band) / float(band)  # distinct, within 0.01 of best; one equals best
    flat = shuffled_flat(rng, n)
    assert check(ctx, score, flat, 22, band_on=True, best=best) == max(22, band)
    assert check(ctx, score, flat, 22, band_on=False, best=best) == 22
    # the band's edge: DoubleEqual is inclusive
    score[inb[0]] = best - 0.01
    check(ctx, score, flat, 22, band_on=True, best=best)


@pytest.mark.parametrize("where", ["on", "between", "off"])
@pytest.mark.parametrize("ns", [13, 33])
def test_near_best_windows(ctx, ns, where):
    """pred = the angular list's test: windows of 5 x 13^2 and 5 x 33^2, the
    best pose on a candidate, between two candidates, and off the window."""
    rng = np.random.default_rng(17 + ns)
    na = 5
    n_cand = na * ns * ns
    x0, y0, step = 31.25, 20.5, 1.0
    sres, mres = 0.1, 0.05
    tol = sres / mres
    bx, by = {"on": (x0 + 5 * step, y0 + 7 * step), "between": (x0 + 5.5 * step, y0 + 7.5 * step),
              "off": (x0 - 10.0, y0 + 3.0)}[where]
    near = (x0, y0, step, ns, bx, by, tol)
    keep = rng.random(n_cand) < 0.8  # a collected list holds part of the window
    flat = rng.permutation(np.nonzero(keep)[0]).astype(np.int64)
    score = rng.permutation(flat.size) / float(flat.size)
    n_near = int(near_pred(flat, near).sum())
    if where == "off":
        assert n_near == 0
    else:
        assert n_near > 22
    for k in (22, 1):
        assert check(ctx, score, flat, k, near=near) == min(k, n_near)
    # fewer near-best hits than K: all of them, whatever their scores
    few = np.nonzero(near_pred(flat, near))[0][:9]
    sub = np.concatenate([few, np.nonzero(~near_pred(flat, near))[0][:500]])
    assert check(ctx, score[sub], flat[sub], 22, near=near) == few.size
    # ties at the near-best set's K-th come along, equal scores outside it do not
    if n_near > 30:
        nb = np.nonzero(near_pred(flat, near))[0]
        order = nb[np.argsort(-score[nb])]
        s2 = score.copy()
        s2[order[21:25]] = s2[order[21]]
        s2[np.nonzero(~near_pred(flat, near))[0][:50]] = s2[order[21]]
        assert check(ctx, s2, flat, 22, near=near) == 25
        assert check(ctx, s2, flat, 22, band_on=True, best=float(s2[order[0]]), near=near) >= 25

