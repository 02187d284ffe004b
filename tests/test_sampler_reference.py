"""The host reference of the GPU sampler (tests/sampler_reference.py) on its own, without a GPU: its generator
against the library's host Philox function, its dim -> (word, slot) map, its draws against scipy's truncnorm and
BOHB's categorical rule -- so that it cannot be wrong in the kernel's own way -- and the GPU cases' coverage and
categorical exclusion counts (tests/test_gpu_sample_draws.py)."""
import numpy as np
import pytest
import scipy.stats as sps

from tests import sampler_reference as R
from tests import test_gpu_sample_draws as T

P_MIN = 1e-4


def test_numpy_philox_equals_the_library_host_function():
    from hpbandster_amd import _native as N
    rs = np.random.RandomState(11)
    ctr = rs.randint(0, 2 ** 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    key = rs.randint(0, 2 ** 32, size=(1000, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0xFFFFFFFF, 0xFFFFFFFF
    ctr[1], key[1] = 0, 0
    got = R.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (1000, 4)
    L = N.lib()
    for k in range(1000):
        c, kk, o = np.ascontiguousarray(ctr[k]), np.ascontiguousarray(key[k]), np.zeros(4, np.uint32)
        N.check(L.hbx_philox4x32_10(N.ptr(c), N.ptr(kk), N.ptr(o)))
        assert np.array_equal(got[k], o), k


def test_word_slot_map_is_one_to_one_up_to_max_d():
    ws = [R.dim_word_slot(d) for d in range(256)]
    assert len(set(ws)) == 256
    assert all(0 <= w < 64 < R.RESERVED_WORD0 and 0 <= s < 4 for w, s in ws)
    assert max(w for w, _ in ws) == 63
    for d in range(256):  # the documented closed form and its period: 16 dims on, 4 words on, the same slot
        assert ws[d] == ((d // 2) % 4 + 4 * (d // 16), 2 * ((d // 8) % 2) + d % 2)
        if d + 16 < 256:
            assert ws[d + 16] == (ws[d][0] + 4, ws[d][1])
    assert ws[8] == (0, 2) and ws[9] == (0, 3)  # D = 9: the first use of slots 2 and 3
    assert ws[16] == (4, 0)                     # D = 17: the first second block of a lane
    assert [ws[d][0] for d in range(0, 8, 2)] == [0, 1, 2, 3]  # 4 lanes, a pair of dims each


def test_counters_wrap_and_split():
    assert R.candidate_counters(2 ** 64 - 2, 4) == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    a = R.blocks(T.SEED, [2 ** 32 - 1, 2 ** 32], 5, 7)
    one = R.philox4x32_10(np.array([[0, 1, 5, 7]]), np.array([[T.SEED & 0xFFFFFFFF, T.SEED >> 32]]))
    assert np.array_equal(a[1], one[0]) and not np.array_equal(a[0], a[1])
    assert np.array_equal(R.datum_index(T.SEED, range(50), 0, 1), np.zeros(50))
    idx = R.datum_index(T.SEED, range(6000), 0, 3)
    assert sps.chisquare(np.bincount(idx, minlength=3)).pvalue > P_MIN


@pytest.mark.parametrize("m,h", [(0.5, 0.2), (0.0, 0.05), (1.0, 0.4), (0.3, 1e-3), (0.9, 0.05), (0.02, 0.4)])
def test_continuous_draws_follow_scipy_truncnorm(m, h):
    D, Nc = 20, 4000  # every dim the same (m, h): each dim's draws are a sample of the one distribution
    r = R.sample(np.full((1, D), m), [0], np.full(D, h), np.zeros(D, int), 3.0, T.SEED, 2 ** 32 - 100, 7, Nc)
    ref = sps.truncnorm(-m / h, (1 - m) / h, loc=m, scale=3.0 * h)
    assert not r.err.any()
    assert r.cands.min() >= m - 3.0 * m - 1e-12 and r.cands.max() <= m + 3.0 * (1 - m) + 1e-12
    assert sps.kstest(r.cands.ravel(), ref.cdf).pvalue > P_MIN  # all dims pooled: also independent enough of each other
    for d in (0, 9, 19):
        assert sps.kstest(r.cands[:, d], ref.cdf).pvalue > P_MIN, d


@pytest.mark.parametrize("m,h,t", [(1, 0.3, 3), (0, 1.7, 2), (2, 1.0, 50), (0, 0.0, 2), (3, 1e-12, 1000), (0, 0.3, 1),
                                   (7, 0.3, 1000)])
def test_categorical_draws_follow_the_rule(m, h, t):
    D, Nc = 8, 6000
    r = R.sample(np.full((1, D), float(m)), [0], np.full(D, h), np.full(D, t), 3.0, T.SEED, 0, 0, Nc)
    x = r.cands.ravel()
    obs = np.bincount(x.astype(np.int64), minlength=t)[:t]
    assert obs.sum() == x.size and np.array_equal(x, np.floor(x))
    keep = min(max(1 - h, 0.0), 1.0)  # rand() < 1 - bw, else a uniform level (the rule of tests/test_gpu_sample.py)
    exp = np.full(t, (1 - keep) / t)
    exp[m] += keep
    if h < 1e-6 or t == 1:
        assert obs[m] == x.size
    elif t <= 50:
        assert sps.chisquare(obs, exp * x.size).pvalue > P_MIN
    else:  # 1000 levels: the kept share, and the resampled levels pooled into 20 bins
        others = x[x != m]
        assert abs((x == m).mean() - exp[m]) < 4 * np.sqrt(exp[m] * (1 - exp[m]) / x.size)
        assert sps.chisquare(np.bincount((others // 50).astype(int), minlength=20)).pvalue > P_MIN


def test_domain_errors_leave_the_other_dims_drawn():
    X = np.array([[0.0, 0.5, np.nan, 0.25, 1.0]])
    r = R.sample(X, [0], [0.0, 0.1, 0.1, 0.0, 0.0], [0] * 5, 3.0, T.SEED, 0, 0, 10)
    assert r.err.all()
    assert np.isnan(r.cands[:, [0, 2, 4]]).all() and np.array_equal(r.domain[0], [True, False, True, False, True])
    assert np.isfinite(r.cands[:, 1]).all() and (r.cands[:, 3] == 0.25).all()


def test_grouped_counters():
    rs = np.random.RandomState(3)
    X, seg, order = rs.rand(12, 3), [0, 5, 5, 12], np.array([4, 0, 2, 1, 3, 6, 5, 4, 3, 2, 1, 0])
    bw, lv, S, C0 = np.full((3, 3), 0.2), [0, 0, 3], 2, 7
    X[:, 2] = np.arange(12) % 3
    out = R.sample_groups(X, seg, order, [3, 1, 9], bw, lv, 3.0, T.SEED, 100, 0, S * C0)
    assert out[1] is None and out[2] is None  # an empty segment, and n_good past the segment
    out = R.sample_groups(X, seg, order, [3, 0, 4], bw, lv, 3.0, T.SEED, 100, 0, S * C0)
    for b, s in ((0, 1), (2, 0), (2, 1)):
        one = R.sample(X[seg[b]:seg[b + 1]], order[seg[b]:][:[3, 0, 4][b]], bw[b], lv, 3.0, T.SEED,
                       100 + (b * S + s) * C0, 0, C0)
        assert np.array_equal(out[b].cands[s * C0:(s + 1) * C0], one.cands)
        assert np.array_equal(out[b].datum[s * C0:(s + 1) * C0], one.datum)


# ---- the GPU cases, as far as they can be checked here --------------------------------------------------------------
def test_gpu_cases_cover_what_they_claim():
    kinds, hs_c, hs_u, ts = set(), set(), set(), set()
    for case in T.CASES:
        lv, bw = T.dim_specs(case[0], case[5])
        for d, (t, h) in enumerate(zip(lv, bw)):
            w, s = R.dim_word_slot(d)
            kinds.add((t > 0, s, w >= 4))
            (hs_u if t else hs_c).add(float(h))
            if t:
                ts.add(int(t))
    assert len(kinds) == 16  # both kinds in every slot of both blocks
    assert hs_c == {0.05, 1e-3, 0.4, 0.0} and hs_u == {0.0, 1e-12, 0.3, 1.0, 1.7} and ts >= {1, 2, 1000}
    assert {len(T.dim_specs(c[0], c[5])[0]) for c in T.CASES} == {1, 2, 5, 7, 8, 9, 10, 16, 17, 18, 32, 33, 40, 256}
    assert {c[1] for c in T.CASES} == {1, 63, 64, 65, 130} and {c[2] for c in T.CASES} == {0, 2 ** 32 - 3, 2 ** 64 - 5}
    assert {c[3] for c in T.CASES} == {0, 7} and {c[4] for c in T.CASES} == {1, 3, 50} and T.SEED >> 32


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: "D%s-Nc%d" % c[:2])
def test_gpu_case_exclusions_and_content(case):
    """The categorical exclusion count of each case's seed (expected 0 with 32-bit uniforms; cap 0.1 %), and that the
    case holds what it is there for"""
    c = T.build_case(case)
    ref = T.reference(c)
    ex, share = T.cat_excluded(ref, c["levels"])
    print("D=%s Nc=%d: categorical draws left out %d" % (case[0], case[1], ex.sum()))
    assert share <= T.CAT_CAP
    assert ex.sum() == 0
    assert np.array_equal(np.isnan(ref.cands), ref.domain)
    cat = c["levels"] > 0
    if cat.any() and len(cat) >= 16:  # kept and resampled draws both present
        moved = ref.cands[:, cat] != ref.m[:, cat]
        assert moved.any() and not moved.all()
    if len(cat) >= 16 and case[4] >= 3:
        assert 0 < ref.err.sum() < ref.err.size  # some domain errors, not only
        assert np.nanmin(ref.ptail) < 1e-2 and np.nanmax(ref.ptail) > 0.4  # tail and centre of the inversion


def test_tail_cases_hold_tail_draws():
    c = T.tail_case()
    ref = T.reference(c)
    assert not ref.err.any() and not ref.clamped.any()
    assert (ref.ptail < 1e-9).sum() >= 130 * 9 // 3 and np.nanmax(np.abs(ref.zs)) <= 30 and (ref.ptail > 1e-3).any()
    assert (ref.zs > 6).any() and (ref.zs < -4).any()  # both the mirrored and the plain lower tail
    assert (ref.ptail < 1e-15).sum() >= 130 * 9 // 6  # the outer range of AS 241 (sqrt(-ln p) > 5)
    mid = (ref.ptail > 1e-11) & (ref.ptail < 1e-6)    # its middle range
    assert mid.sum() >= 130 * 9 // 6
    ref = T.reference(T.rare_tail_case())
    n = int((ref.ptail < 1e-6).sum())
    print("rare tail: %d draws with min(p, 1 - p) < 1e-6" % n)
    assert n >= 1
