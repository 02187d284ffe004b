"""The staged top-k's selection rule (hbx_topk.hip "Staged scoring") restated in numpy (tools/staged_survivors.py:
seed band around the (k+1)-th largest l, U_(k+1) over the seeds, survivors by their l-only bound, rank the
evaluated) against brute force over every candidate, on seeded random (l, g) arrays with values below the 1e-8
clamp, NaN and duplicates; the helpers' argument checks; the native size helpers.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    spec = importlib.util.spec_from_file_location("staged_survivors", os.path.join(ROOT, "tools", "staged_survivors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _arrays(seed, n):
    """l and g over 12 decades around the clamp, a third of them below it, with NaN in both and repeated
    (l, g) pairs: exact score ties at scattered indices."""
    rs = np.random.RandomState(seed)
    l = 10.0 ** rs.uniform(-14, -2, size=n)
    g = 10.0 ** rs.uniform(-14, -2, size=n)
    l[rs.rand(n) < 0.05] = np.nan
    g[rs.rand(n) < 0.05] = np.nan
    l[rs.rand(n) < 0.05] = 0.0
    dup = rs.randint(0, n, size=n // 5)
    src = rs.randint(0, n, size=n // 5)
    l[dup], g[dup] = l[src], g[src]
    return l, g


@pytest.mark.parametrize("seed", range(12))
def test_selection_equals_brute_force(P, seed):
    """Every k, with the whole band as seeds and with random subsets of at least k + 1 of its members: the same
    first k by (score, index) as ranking everything, and g is read for the evaluated candidates only."""
    rs = np.random.RandomState(100 + seed)
    n = int(rs.choice([40, 300, 2000]))
    l, g = _arrays(seed, n)
    for k in (1, 2, 7, 64, 1024):
        want = P.brute_topk(l, g, k)
        L, band = P.topk_seed_band(l, k)
        subsets = [None]
        if len(band) > k + 1:
            subsets += [np.sort(rs.choice(band, size=int(rs.randint(k + 1, len(band) + 1)), replace=False))
                        for _ in range(3)]
        for seeds in subsets:
            asked = []

            def g_of(idx):
                asked.extend(np.asarray(idx).tolist())
                return g[idx]
            r = P.topk_select(l, g_of, k, seeds=seeds)
            np.testing.assert_array_equal(r["top"], want, err_msg=str((seed, n, k)))
            assert sorted(asked) == sorted(r["evaluated"].tolist()) and len(set(asked)) == len(asked)
            s = P.bohb_scores(l, g)
            np.testing.assert_array_equal(r["scores"], s[want])
            pruned = np.setdiff1d(np.nonzero(~np.isnan(l))[0], r["evaluated"])
            if len(pruned):  # each pruned candidate is strictly behind k + 1 others
                assert np.sum(s[r["evaluated"]] < s[pruned].min()) >= k + 1


def test_prunes_and_no_threshold(P):
    """A pool where l rules nearly everything out, and one with fewer than k + 1 candidates that have an l."""
    rs = np.random.RandomState(5)
    l = np.concatenate([10.0 ** rs.uniform(-3, -2, size=50), 10.0 ** rs.uniform(-14, -9, size=950)])
    g = 10.0 ** rs.uniform(-8, -6, size=1000)
    r = P.topk_select(l, lambda i: g[i], 8)
    assert len(r["evaluated"]) <= 50 and r["U"] < 1.0
    np.testing.assert_array_equal(r["top"], P.brute_topk(l, g, 8))
    l2 = np.full(20, np.nan)
    l2[[3, 7, 11]] = [1e-3, 1e-12, 1e-5]
    g2 = np.full(20, 1e-7)
    L, band = P.topk_seed_band(l2, 3)
    assert L is None and band.tolist() == [3, 7, 11]
    r = P.topk_select(l2, lambda i: g2[i], 3)
    assert r["U"] == float("inf") and r["top"].tolist() == [3, 11, 7]
    every_one = P.topk_select(np.full(30, 1e-12), lambda i: np.full(len(i), 1e-12), 4)
    assert every_one["top"].tolist() == [0, 1, 2, 3] and len(every_one["evaluated"]) == 30  # ties survive '<='


def test_argument_checks(P):
    l = 10.0 ** np.linspace(-12, -2, 100)
    g = np.full(100, 1e-6)
    for bad in (0, 1025, -1, 2.5):
        with pytest.raises(ValueError):
            P.topk_seed_band(l, bad)
        with pytest.raises(ValueError):
            P.topk_u(np.ones(4), bad)
    with pytest.raises(ValueError):
        P.topk_seed_band(np.ones((3, 3)), 1)
    L, band = P.topk_seed_band(l, 4)
    with pytest.raises(ValueError):  # outside the band
        P.topk_select(l, lambda i: g[i], 4, seeds=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError):  # fewer than k + 1 seeds from a band that holds them
        P.topk_select(l, lambda i: g[i], 4, seeds=band[:3])
    assert P.topk_u([3.0, 1.0, np.nan, 2.0], 1) == 2.0 and P.topk_u([1.0], 1) == float("inf")
    assert np.isnan(P.bohb_scores([np.nan], [1.0])[0]) and P.bohb_scores([1e-3], [np.nan])[0] == 1e-8 / 1e-3


def test_native_size_helpers():
    """The staged top-k keeps the result block and the workspace: 16 + 40 k bytes, and the argmin's workspace
    plus the select's histograms."""
    from hpbandster_amd import _native as N
    L = N.lib()
    for k in (1, 64, 1024):
        assert L.hbx_kde_topk_result_bytes(k) == 16 + 40 * k
        for nc, nmax in ((700, 1000), (4097, 350), (1000000, 10000)):
            assert L.hbx_kde_topk_workspace_bytes(nc, k, nmax) == L.hbx_kde_workspace_bytes(nc, nmax) + 4096
    for bad in (0, 1025):
        assert L.hbx_kde_topk_result_bytes(bad) == -1 and L.hbx_kde_topk_workspace_bytes(700, bad, 1000) == -1
    assert L.hbx_kde_topk_workspace_bytes(-1, 4, 1000) == -1
