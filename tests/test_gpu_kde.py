"""GPU parity: the HIP KDE fit / scoring / acquisition against the reference's golden fixtures.

Tolerances (north star): chosen indices and promotion masks bit-exact; fp32 log-densities within
1e-5 relative of the reference fp64 path (|d ln pdf| <= 1e-5 * max(1, |ln pdf|)); the exact fp64
path bit-identical to the reference (statsmodels on the pinned numpy 1.26.4, whose SVML exp the engine
restates).
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests import golden_cases as G

pytestmark = pytest.mark.gpu


def _ref_log(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, np.log(p), np.where(np.isnan(p), np.nan, -np.inf))


def _pair_from_fixture(c):
    from hpbandster_amd import kde
    X = c["X"]
    return kde.fit_pair_from_rows(X, c["good_idx"], c["bad_idx"], c["var_type"], c["bw_good"], c["bw_bad"],
                                  c["nlev_good"], c["nlev_bad"])


@pytest.mark.parametrize("name", G.kde_case_names())
def test_fit_bit_exact(device, name):
    from hpbandster_amd import kde
    c = G.load_kde_case(name)
    pair = kde.fit_pair(c["X"], c["eff_losses"], c["var_type"], int(c["min_points"]), device=device)
    assert pair is not None
    good_rows = pair.good.rows_dev.cpu().numpy()
    bad_rows = pair.bad.rows_dev.cpu().numpy()
    # the reference's rows in its order, tied losses (crashed +inf, quantised) included: the refit's
    # argsort is numpy 1.26.4's (hbx_npsort.h), so the bandwidths' summation order is the reference's too
    np.testing.assert_array_equal(good_rows, c["good_idx"])
    np.testing.assert_array_equal(bad_rows, c["bad_idx"])
    np.testing.assert_array_equal(pair.good.bw, c["bw_good"])
    np.testing.assert_array_equal(pair.bad.bw, c["bw_bad"])
    np.testing.assert_array_equal(pair.good.nlev, c["nlev_good"])
    np.testing.assert_array_equal(pair.bad.nlev, c["nlev_bad"])


# scoring kernel families, chosen when a KDE is prepared: "h32" the default (f16 matrix-core exponent
# on 32x32 tiles where the shape allows it, hbx_score_h32.hip), "h16" its 16x16-tile form
# (hbx_score_h.hip, HBX_H32=0), "f32" the f32-MFMA fallback kernels everywhere (HBX_HMODE=0)
KERNELS = {"h32": {"HBX_HMODE": "1", "HBX_H32": "1"}, "h16": {"HBX_HMODE": "1", "HBX_H32": "0"},
           "f32": {"HBX_HMODE": "0", "HBX_H32": "1"}}


def _kernel_env(monkeypatch, kernel):
    for k, v in KERNELS[kernel].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", G.kde_case_names())
def test_logpdf_fp32_within_tolerance(device, name, kernel, monkeypatch):
    """Every kernel family's fp32 ln-pdf estimates within the north-star 1e-5 of the reference."""
    _kernel_env(monkeypatch, kernel)
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    C = c["cands"]
    res, logl, logg = pair.acquire(C, logs=True)
    for est, ref, kde_ in ((logl, c["pdf_l"], pair.good), (logg, c["pdf_g"], pair.bad)):
        # reference ln pdf from the oracle's fp64 log-space restatement (covers pdf underflow)
        lref = O.log_pdf_many(c["X"][kde_.rows_dev.cpu().numpy()], kde_.bw, c["var_type"], C, kde_.nlev)
        nan = np.isnan(lref)
        assert np.array_equal(np.isnan(est), nan), name
        neg = np.isneginf(lref)
        assert np.all(np.isneginf(est[neg])), name
        fin = np.isfinite(lref)
        err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.max(initial=0.0) <= 1e-5, (name, err.max())
        # and against the reference's own pdf values where they are representable
        lr = _ref_log(ref)
        ok = np.isfinite(lr) & (ref > 1e-300)
        err2 = np.abs(est[ok] - lr[ok]) / np.maximum(1.0, np.abs(lr[ok]))
        assert err2.max(initial=0.0) <= 1e-5, (name, err2.max())


@pytest.mark.parametrize("name", G.kde_case_names())
def test_exact_pdf_bit_identical_to_reference(device, name):
    """The fp64 re-score against the reference's own KDEMultivariate.pdf outputs: bit for bit (same
    float64 operations in the same order, numpy's exp restated exactly)."""
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    C = c["cands"][:128]
    l = np.atleast_1d(pair.good.pdf(C))
    g = np.atleast_1d(pair.bad.pdf(C))
    np.testing.assert_array_equal(l, c["pdf_l"][:len(C)])
    np.testing.assert_array_equal(g, c["pdf_g"][:len(C)])


@pytest.mark.parametrize("name", G.kde_case_names())
def test_logpdf_contract_against_reference(device, name):
    """DeviceKDE.logpdf (fp32 estimate where its bound allows, fp64 log space / exact pdf otherwise)
    within the north-star 1e-5 of the reference's own ln pdf wherever that is finite; the fp64
    log-space kernel alone within 1e-12 of it (KDEs with positive factors)."""
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    C = c["cands"][:128]
    for k, ref in ((pair.good, c["pdf_l"][:len(C)]), (pair.bad, c["pdf_g"][:len(C)])):
        with np.errstate(divide="ignore", invalid="ignore"):
            lref = np.log(ref)
        fin = np.isfinite(lref)
        lp = k.logpdf(C)
        assert np.array_equal(np.isnan(lp), np.isnan(lref))
        assert (np.abs(lp[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))).max(initial=0.0) <= 1e-5
        if not (k.has_neg or k.nan_all or k.nconst):
            lx = k._logpdf_exact(np.ascontiguousarray(C), None)
            assert (np.abs(lx[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))).max(initial=0.0) <= 1e-12


def test_np_exp_known_answers(device):
    """The device restatement of numpy's float64 exp against numpy 1.26.4's own outputs (the pinned
    reference interpreter), 2e4 inputs over every range including subnormal results and overflow."""
    import torch
    from hpbandster_amd import _native as N
    z = np.load(G.GOLDEN + "/np_exp.npz")
    x = torch.from_numpy(z["x"]).to(device)
    y = torch.empty_like(x)
    N.check(N.lib().hbx_np_exp(N.ptr(x), x.numel(), N.ptr(y), N.stream_handle(None, device)))
    np.testing.assert_array_equal(y.cpu().numpy().view(np.uint64), z["y"].view(np.uint64))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", G.kde_case_names())
def test_acquire_chosen_index_bit_exact(device, name, kernel, monkeypatch):
    _kernel_env(monkeypatch, kernel)
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    res = pair.acquire(c["cands"])
    assert res.index == c["chosen"], (name, res, c["chosen"])
    if res.index >= 0:
        assert res.score == c["scores"][res.index]  # the reference's exact score, bit for bit
        assert res.shortlist >= 1


@pytest.mark.parametrize("name", G.kde_case_names())
def test_acquire_sharded_indices(device, name):
    """Sharding the candidates (index_base) and reducing the local winners gives the same index."""
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    C = c["cands"]
    cuts = [0, len(C) // 3, (2 * len(C)) // 3, len(C)]
    best = (np.inf, -1)
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = pair.acquire(C[a:b], index_base=a)
        if r.index >= 0 and (r.score < best[0] or (r.score == best[0] and r.index < best[1])):
            best = (r.score, r.index)
    assert best[1] == c["chosen"]


@pytest.mark.parametrize("name", G.getcfg_names())
def test_get_config_candidates_select_like_reference(device, name):
    """Candidate sets the reference's BOHB.get_config generated and scored: same winner."""
    from hpbandster_amd import kde
    g = G.load_getcfg(name)
    dc, du, lv, n = g["dc"], g["du"], g["levels"], g["n_obs"]
    from hpbandster_amd import synthetic as S
    X = S.make_observations(n, dc, du, lv if len(lv) > 1 else int(lv[0]))
    L = S.make_losses(n)
    pair = kde.fit_pair(X, L, "c" * dc + "u" * du, dc + du + 1, device=device)
    for r in g["records"]:
        if not bool(r["model_based"]):
            continue
        res = pair.acquire(r["cands"])
        assert res.index == int(r["chosen"])
        np.testing.assert_array_equal(r["cands"][res.index], r["vec"])


def test_acquire_edge_cases(device):
    c = G.load_kde_case("d1")
    pair = _pair_from_fixture(c)
    r = pair.acquire(np.zeros((0, 1)))
    assert r.index == -1 and r.shortlist == 0
    r = pair.acquire(c["cands"][:1])
    assert r.index == 0
    # all-NaN candidates -> no finite score -> -1 (bohb.py:154-157 falls back to random)
    r = pair.acquire(np.full((5, 1), np.nan))
    assert r.index == -1
    # duplicates of the winner: first index wins
    w = c["cands"][c["chosen"]]
    C = np.vstack([c["cands"], w[None, :], w[None, :]])
    r = pair.acquire(C)
    assert r.index == c["chosen"]


def test_rescue_path_far_candidates(device):
    """Candidates whose every term underflows the static fp32 bound take the two-pass rescue."""
    from hpbandster_amd import kde
    rs = np.random.RandomState(3)
    X = 0.5 + 1e-3 * rs.rand(60, 2)
    L = rs.rand(60)
    pair = kde.fit_pair(X, L, "cc", 3, device=device)
    C = np.array([[0.5, 0.5], [0.505, 0.5], [0.52, 0.5], [0.9, 0.1], [0.501, 0.5005]])
    res, logl, logg = pair.acquire(C, logs=True)
    ref_l = O.log_pdf_many(pair.good.data, pair.good.bw, "cc", C)
    fin = np.isfinite(ref_l)
    assert fin.sum() >= 3
    err = np.abs(logl[fin] - ref_l[fin]) / np.maximum(1, np.abs(ref_l[fin]))
    assert err.max() <= 1e-5
    l = O.pdf_many(pair.good.data, pair.good.bw, "cc", C)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, "cc", C)
    assert res.index == O.select(l, g)[0]


@pytest.mark.parametrize("n_obs", [10000, 20000])
def test_exact_split_units_match_whole_sum(device, n_obs):
    """The acquisition's exact re-score spreads one candidate's observations over tree units (one
    block each) and recombines them; DeviceKDE.pdf sums every unit in one block.  Same additions in
    the same order -> bit-identical pdfs; and both bit-identical to the C oracle's restatement of the
    reference arithmetic (numpy sums over 8192-element buffers: n=20000 has three)."""
    from oracle import c_oracle
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    X = S.make_observations(n_obs, 24, 8, 4)
    L = S.make_losses(n_obs)
    vt = S.var_type_string(24, 8)
    pair = kde.fit_pair(X, L, vt, 33, device=device)
    C = S.make_candidates(64, 24, 8, 4)
    res = pair.acquire(C)
    assert res.index >= 0
    w = C[res.index:res.index + 1]
    assert np.asarray(pair.good.pdf(w)).item() == res.pdf_l
    assert np.asarray(pair.bad.pdf(w)).item() == res.pdf_g
    l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
    g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    assert (res.pdf_l, res.pdf_g) == (l[res.index], g[res.index])
    assert res.index == O.select(l, g)[0]


def test_hmode_falls_back_when_cj_exceeds_f16_range(device):
    """A far outlier among tightly clustered observations makes |C_j| = |X'_j|^2 + ... exceed the
    f16 range of the C_j pieces: that KDE is prepared for the f32-MFMA kernel instead, the other one
    stays on the f16 kernel, and the acquisition still matches the reference."""
    from hpbandster_amd import kde
    rs = np.random.RandomState(11)
    n, D = 8500, 16
    X = 0.5 + 1e-3 * rs.rand(n, D)
    X[17] = 0.0  # the outlier
    L = rs.rand(n)
    L[17] = np.sort(L)[n // 2]  # mid loss: lands in the bad KDE only
    vt = "c" * D
    pair = kde.fit_pair(X, L, vt, D + 1, device=device)
    assert 17 in set(pair.bad.rows_dev.cpu().numpy()) and 17 not in set(pair.good.rows_dev.cpu().numpy())
    assert (pair.good.variant >> 4) & 1 == 1  # f16 matrix-core kernel
    assert (pair.bad.variant >> 4) & 1 == 0   # fallback: f32 MFMA
    C = np.vstack([0.5 + 1e-3 * rs.rand(200, D), 0.02 * rs.rand(56, D)])
    res, logl, logg = pair.acquire(C, logs=True)
    for est, k in ((logl, pair.good), (logg, pair.bad)):
        lref = O.log_pdf_many(k.data, k.bw, vt, C)
        fin = np.isfinite(lref)
        assert np.array_equal(np.isfinite(est), fin)
        err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        # candidates inside the cluster: the north-star tolerance
        assert err[:fin[:200].sum()].max() <= 1e-5
        # candidates ~100 bandwidths from the KDE centre next to the outlier: the fp32 expansion
        # -|x'|^2 - |X'|^2 + 2x'.X' cancels terms of ~1e5 (documented in DESIGN.md); the estimate is
        # still within its rigorous bound, which is what keeps the selection exact
        assert err.max() <= 5e-2
        # DeviceKDE.logpdf keeps the contract everywhere: estimates inside it, exact pdfs for the rest
        lp = k.logpdf(C)
        assert np.array_equal(np.isfinite(lp), fin)
        assert (np.abs(lp[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))).max() <= 1e-5
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C)
    assert res.index == O.select(l, g)[0]


@pytest.mark.parametrize("dc,levels", [
    (20, [3, 5, 2, 3, 4, 3]),   # odd level counts: one-hot positions padded per dim, sparse (2:4) product
    (24, [4, 4, 4]),            # 12 positions -> one dense f16 one-hot step (kc = 1)
    (30, [4] * 16),             # 64 positions -> kc = 4, two sparse steps
    (17, []),                   # continuous only on the f16 kernel
])
@pytest.mark.parametrize("kernel", ["h32", "h16"])
def test_hmode_categorical_layouts_match_oracle(device, dc, levels, kernel, monkeypatch):
    """The f16 matrix-core kernels over one-hot layouts the bench shape does not use (kc = 4 at
    dc_pad = 32 is beyond the 32x32 kernel's register budget: the 16x16 kernel runs it either way)."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    _kernel_env(monkeypatch, kernel)
    du = len(levels)
    n = 2000
    X = S.make_observations(n, dc, du, levels if du else 2, seed=21)
    L = S.make_losses(n, seed=22)
    vt = S.var_type_string(dc, du)
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    assert (pair.good.variant >> 4) & 1 == 1 and (pair.bad.variant >> 4) & 1 == 1
    want32 = kernel == "h32" and not (dc == 30 and du == 16)
    for k in (pair.good, pair.bad):  # signed sums (a factor 1 - h < 0) included
        assert (k.variant >> 6) & 1 == want32
    C = S.make_candidates(384, dc, du, levels if du else 2, seed=23)
    res, logl, logg = pair.acquire(C, logs=True)
    for est, k in ((logl, pair.good), (logg, pair.bad)):
        lref = O.log_pdf_many(k.data, k.bw, vt, C, k.nlev)
        fin = np.isfinite(lref)
        assert np.array_equal(np.isfinite(est), fin)
        err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        # the north-star tolerance (1e-5) is stated at D <= 32; beyond it the fp32 expansion
        # -|x'|^2 - |X'|^2 + 2x'.X' cancels larger terms (error ~ 2^-24 sum|terms|), still inside
        # the rigorous per-candidate bound that keeps the selection exact
        assert err.max() <= (1e-5 if dc + du <= 32 else 3e-5), err.max()
        assert np.median(err) <= 1e-6
        lp = k.logpdf(C)  # the contract at every D
        assert (np.abs(lp[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))).max() <= 1e-5
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    assert res.index == O.select(l, g)[0]


def test_clamped_ties_score_one_first_index(device):
    """Candidates whose l and g are both below 1e-8 score exactly max(1e-8,g)/max(l,1e-8) = 1
    (bohb.py:129) and tie; the first of them wins unless some candidate scores below 1.  Only the
    first tie needs the exact re-score, so the shortlist stays small (BOHB's sampler at D=32 puts
    most candidates there)."""
    from hpbandster_amd import kde
    rs = np.random.RandomState(8)
    D = 12
    X = rs.rand(400, D)
    L = rs.rand(400)
    pair = kde.fit_pair(X, L, "c" * D, D + 1, device=device)
    far = 5.0 + rs.rand(3000, D)  # pdf underflows for both KDEs
    res = pair.acquire(far)
    assert res.index == 0 and res.score == 1.0
    assert res.shortlist <= 2
    near = pair.good.data[:3] + 1e-3
    C = np.vstack([far[:1000], near, far[1000:]])
    l = O.pdf_many(pair.good.data, pair.good.bw, "c" * D, C)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, "c" * D, C)
    want, scores = O.select(l, g)
    res = pair.acquire(C)
    assert res.index == want
    assert res.shortlist <= 10
    # batched: a far-only segment and a mixed one
    rb = pair.acquire_batch(np.vstack([far[:500], C[800:1300]]), 500)
    assert rb[0].index == 0 and rb[0].score == 1.0
    assert rb[1].index == O.py_argmin(scores[800:1300])


@pytest.mark.parametrize("kernel", ["h32", "h16"])
@pytest.mark.parametrize("shape", [(24, 8, 4, 3000, 20011), (32, 0, 0, 1000, 777), (16, 8, 3, 400, 65)])
def test_pair_launch_identical_to_two_launches(device, shape, kernel, monkeypatch):
    """l and g scored by one pair launch (the default) against two single launches
    (HBX_SCORE_PAIR=0): the same kernel body per block, so the ln-pdf estimates and the acquisition
    record are bit-identical; the chosen index is the oracle's."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du, lev, n_obs, n_cand = shape
    _kernel_env(monkeypatch, kernel)
    X = S.make_observations(n_obs, dc, du, lev)
    L = S.make_losses(n_obs)
    vt = S.var_type_string(dc, du)
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    C = S.make_candidates(n_cand, dc, du, lev)
    monkeypatch.setenv("HBX_SCORE_PAIR", "1")
    r1, l1, g1 = pair.acquire(C, logs=True)
    monkeypatch.setenv("HBX_SCORE_PAIR", "0")
    r0, l0, g0 = pair.acquire(C, logs=True)
    assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32))
    assert np.array_equal(g1.view(np.uint32), g0.view(np.uint32))
    assert (r1.index, r1.pdf_l, r1.pdf_g, r1.shortlist) == (r0.index, r0.pdf_l, r0.pdf_g, r0.shortlist)
    if n_cand <= 1000:
        l = O.pdf_many(pair.good.data, pair.good.bw, vt, C)
        g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C)
        assert r1.index == O.select(l, g)[0]


@pytest.mark.parametrize("name", ["neartie_c", "neartie_m"])
def test_near_ties_pinned_and_process(device, name):
    """Near ties (copies of the reference's best candidate moved by a few ulps, exact duplicates).
    Pinned policy: the reference's own pick (its exact scores bit for bit), the near set flagged.
    Process policy: the pick this process's numpy makes (numpy restatement run here), single and
    batched, and through the two-stage sharded exchange at world size 1."""
    from hpbandster_amd.kde import ACQ_NEAR_TIE, ACQ_RESOLVED
    c = G.load_kde_case(name)
    pair = _pair_from_fixture(c)
    C = c["cands"]
    res = pair.acquire(C)
    assert res.index == c["chosen"] and res.score == c["scores"][c["chosen"]]
    assert res.flags & ACQ_NEAR_TIE and res.near > 1
    l = O.pdf_many(pair.good.data, pair.good.bw, c["var_type"], C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, c["var_type"], C, pair.bad.nlev)
    want = O.select(l, g)[0]
    rp = pair.acquire(C, ties="process")
    assert rp.index == want and rp.flags & ACQ_RESOLVED
    assert (rp.pdf_l, rp.pdf_g) == (l[want], g[want])
    rb = pair.acquire_batch(C, C.shape[0], ties="process")
    assert rb[0].index == want
    assert pair.acquire_batch(C, C.shape[0])[0].index == c["chosen"]


@pytest.mark.parametrize("dc,du,lev", [(70, 0, 0), (3, 33, 3)])
def test_exact_only_outside_scoring_buckets(device, dc, du, lev):
    """Spaces beyond the fp32 scoring buckets (> 64 continuous or > 32 categorical dims) run
    exact-only: every candidate re-scored in fp64 -- pick and pdfs equal the C oracle's exact
    (reference-arithmetic) ones; refit through the one-call path; batched too."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    from oracle import c_oracle
    D = dc + du
    X = S.make_observations(4 * D + 40, dc, du, lev)
    L = S.make_losses(X.shape[0])
    vt = S.var_type_string(dc, du)
    pair = kde.fit_pair(X, L, vt, D + 1, device=device)
    assert pair.good.exact_only and pair.bad.exact_only
    C = S.make_candidates(300, dc, du, lev)
    near = X[pair.good.rows_dev.cpu().numpy()[:50]].copy()  # near the good observations
    near[:, :dc] += 1e-3
    C[:near.shape[0]] = near
    res, logl, logg = pair.acquire(C, logs=True)
    l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
    g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    want, scores = O.select(l, g)
    assert res.index == want and res.shortlist == C.shape[0]
    if want >= 0:
        assert (res.pdf_l, res.pdf_g) == (l[want], g[want])
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(logl, np.log(l).astype(np.float32), rtol=1e-6)
    rb = pair.acquire_batch(C, 100)
    for b in range(3):
        assert rb[b].index == O.py_argmin(scores[100 * b:100 * b + 100])


def test_h32_kernel_choice_and_large_shift_rescue(device, monkeypatch):
    """The bench shape (24c + 8u, 4 levels) runs the 32x32-tile kernel (variant bit 6) and, with
    HBX_H32=0, the 16x16 one.  Candidates thousands of bandwidths out have a shifted c_i beyond the
    range of its three f16 pieces (H32_CMAX): they take the rescue pass and still match the oracle's
    log-space pdf; both kernels pick the oracle's winner."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(3000, 24, 8, 4, seed=31)
    L = S.make_losses(3000, seed=32)
    C = S.make_candidates(512, 24, 8, 4, seed=33)
    C[5, 0] = 1000.0
    C[77, 3] = -400.0
    C[300, 23] = 2500.0
    for kernel, bit in (("h32", 1), ("h16", 0)):
        _kernel_env(monkeypatch, kernel)
        pair = kde.fit_pair(X, L, vt, 33, device=device)
        assert (pair.good.variant >> 4) & 1 == 1 and (pair.bad.variant >> 4) & 1 == 1
        assert not pair.bad.has_neg and pair.good.has_neg  # one KDE of each kind
        for k in (pair.good, pair.bad):
            assert (k.variant >> 6) & 1 == bit
        res, logl, logg = pair.acquire(C, logs=True)
        for est, k in ((logl, pair.good), (logg, pair.bad)):
            lref = O.log_pdf_many(k.data, k.bw, vt, C, k.nlev)
            fin = np.isfinite(lref)
            if not k.has_neg:  # (a signed KDE's far pdf may be <= 0: -inf)
                assert fin[[5, 77, 300]].all()
            assert np.array_equal(np.isfinite(est), fin)
            err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
            assert err.max() <= 1e-5, (kernel, err.max())
        l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
        g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
        assert res.index == O.select(l, g)[0]
        fast = pair.acquire(C)  # the FAST instances (the signed good KDE's too)
        assert (fast.index, fast.score, fast.pdf_l, fast.pdf_g) == (res.index, res.score, res.pdf_l, res.pdf_g)


@pytest.mark.parametrize("dc,du", [(8, 4), (6, 8), (8, 12), (16, 0), (12, 4), (16, 8), (24, 4), (32, 0), (16, 12),
                                   (32, 4)])
def test_h32_every_instance_matches_oracle(device, dc, du):
    """Every (continuous K-steps, one-hot steps) instance of the 32x32-tile kernel the bench shape does
    not use -- nsc = dc_pad / 8, kp = ceil(one-hot positions / 32) with 3-level dims padded to 4
    positions -- on 2000 observations (chunks partly filled) and 700 candidates (a partial block):
    the precise instance's ln-pdf estimates within 1e-5 of the oracle's log-space restatement, the
    oracle's winner from it and from the acquisition's FAST instance (one-hot lo parts in the bound),
    whose result record equals the precise one's in index, score and pdfs."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    n, lev = 2000, 3
    X = S.make_observations(n, dc, du, lev, seed=41)
    L = S.make_losses(n, seed=42)
    vt = S.var_type_string(dc, du)
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    assert not pair.bad.has_neg
    assert (pair.bad.variant >> 6) & 1 == 1  # the 32x32 kernel
    C = S.make_candidates(700, dc, du, lev, seed=43)
    res, logl, logg = pair.acquire(C, logs=True)
    for est, k in ((logl, pair.good), (logg, pair.bad)):
        lref = O.log_pdf_many(k.data, k.bw, vt, C, k.nlev)
        fin = np.isfinite(lref)
        assert np.array_equal(np.isfinite(est), fin)
        err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.max() <= 1e-5, err.max()
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    assert res.index == O.select(l, g)[0]
    fast = pair.acquire(C)  # no ln-pdf estimates requested: the FAST scoring instance
    assert fast.index == res.index
    assert (fast.score, fast.pdf_l, fast.pdf_g) == (res.score, res.pdf_l, res.pdf_g)


@pytest.mark.parametrize("dc,du,lev,kc", [
    (0, 4, 20, 0),   # VALU matching (more than the 64 one-hot positions the matrix cores take): dc_pad 0, du_pad 4
    (33, 8, 12, 0),  # ... dc_pad 64, du_pad 8
    (3, 17, 3, 0),   # ... dc_pad 4, du_pad 32
    (12, 16, 3, 4),  # one-hot: dc_pad 16, kc 4
    (32, 4, 3, 1),   # ... dc_pad 32, kc 1
    (33, 8, 3, 2),   # ... dc_pad 64, kc 2
])
def test_f32_families_remaining_buckets_match_oracle(device, dc, du, lev, kc, monkeypatch):
    """The f32-MFMA fallback families (HBX_HMODE=0: VALU categorical matching, kc = 0, or the one-hot product)
    in the buckets no other test selects, modelled on test_h32_every_instance_matches_oracle: 200 observations
    (the good set under one 64-observation chunk, the bad set two chunks and a partial one) and 600 candidates
    (a full and a partial block).  The ln-pdf estimates within 1e-5 of the oracle's log-space restatement, the
    oracle's winner, the same record with and without estimates requested, and the ln-pdf contract through
    DeviceKDE.logpdf (its direct-difference and tiled fp64 kernels at 16 and 32 categorical slots)."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    _kernel_env(monkeypatch, "f32")
    n = 200
    X = S.make_observations(n, dc, du, lev, seed=71)
    L = S.make_losses(n, seed=72)
    C = S.make_candidates(600, dc, du, lev, seed=73)
    vt = S.var_type_string(dc, du)
    # the reference's split and bandwidths; over 12 and 20 levels the normal-reference rule gives categorical
    # bandwidths above 1 (signed sums): those dims get bandwidths below 1 instead
    g_idx, b_idx = O.bohb_split(X, L, dc + du + 1)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    if lev > 3:
        bwg[dc:], bwb[dc:] = np.linspace(0.2, 0.5, du), np.linspace(0.6, 0.3, du)
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt), device=device)
    for k in (pair.good, pair.bad):
        assert not k.has_neg
        assert (k.variant >> 4) & 1 == 0 and k.kc == kc  # not the f16 matrix-core kernels; the family
    res, logl, logg = pair.acquire(C, logs=True)
    for est, k in ((logl, pair.good), (logg, pair.bad)):
        lref = O.log_pdf_many(k.data, k.bw, vt, C, k.nlev)
        fin = np.isfinite(lref)
        assert np.array_equal(np.isfinite(est), fin)
        err = np.abs(est[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.max() <= 1e-5, err.max()
        lp = k.logpdf(C)
        errc = np.abs(lp[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert errc.max() <= 1e-5, errc.max()
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    assert res.index == O.select(l, g)[0]
    fast = pair.acquire(C)
    assert fast.index == res.index
    assert (fast.score, fast.pdf_l, fast.pdf_g) == (res.score, res.pdf_l, res.pdf_g)


def test_fast_instance_extreme_categorical_bandwidths(device):
    """The acquisition's FAST instance (one-hot lo parts in the bound) where the categorical deltas are
    large and far from f16 values: bandwidths from 1e-3 to 0.7 on 8 four-level dims (|delta| up to
    ~11.5 log2 units, lo parts up to 2^-8 each).  The winner is the oracle's and the record equals the
    precise instance's."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du, n = 24, 8, 3000
    X = S.make_observations(n, dc, du, 4, seed=51)
    L = S.make_losses(n, seed=52)
    vt = S.var_type_string(dc, du)
    g_idx, b_idx = O.bohb_split(X, L, dc + du + 1)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    cat = np.array([1e-3, 0.003, 0.01, 0.05, 0.2, 0.37, 0.5, 0.7])
    bwg[dc:], bwb[dc:] = cat, cat[::-1]
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt))
    assert (pair.bad.variant >> 6) & 1 == 1 and not pair.bad.has_neg and not pair.good.has_neg
    C = S.make_candidates(700, dc, du, 4, seed=53)
    C[::2, dc:] = X[g_idx[np.arange(350) % len(g_idx)], dc:]  # half the candidates match a good row's levels
    fast = pair.acquire(C)
    res, _, _ = pair.acquire(C, logs=True)
    l = O.pdf_many(X[g_idx], bwg, vt, C, O.num_levels(X[g_idx], vt))
    g = O.pdf_many(X[b_idx], bwb, vt, C, O.num_levels(X[b_idx], vt))
    assert fast.index == res.index == O.select(l, g)[0]
    assert (fast.score, fast.pdf_l, fast.pdf_g) == (res.score, res.pdf_l, res.pdf_g)


def test_fast_and_precise_records_agree_on_random_shapes(device):
    """200 random (continuous, categorical, levels, observations, bandwidth scale) shapes -- small
    observation counts give signed KDEs -- and 400 candidates each, a third of them on observed
    categorical levels: the acquisition through the FAST scoring instance returns the precise instance's
    record (index, score, pdfs); every tenth shape also against the oracle's winner."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    rs = np.random.RandomState(71)
    for case in range(200):
        dc, du = int(rs.randint(5, 33)), int(rs.randint(1, 13))
        lev = int(rs.randint(2, 7))
        n = int(rs.choice([60, 150, 400, 1200, 2500]))
        vt = S.var_type_string(dc, du)
        X = S.make_observations(n, dc, du, lev, seed=1000 + case)
        L = S.make_losses(n, seed=2000 + case)
        g_idx, b_idx = O.bohb_split(X, L, dc + du + 1) or (None, None)
        if g_idx is None:
            continue
        scale = float(rs.choice([0.3, 1.0, 2.5]))
        bwg, bwb = O.normal_reference_bw(X[g_idx]) * scale, O.normal_reference_bw(X[b_idx]) * scale
        bwg, bwb = np.clip(bwg, 1e-3, None), np.clip(bwb, 1e-3, None)
        nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)
        pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, nlg, nlb)
        C = S.make_candidates(400, dc, du, lev, seed=3000 + case)
        C[::3, dc:] = X[g_idx[np.arange(len(C[::3])) % len(g_idx)], dc:]
        fast = pair.acquire(C)
        res, _, _ = pair.acquire(C, logs=True)
        assert (fast.index, fast.score, fast.pdf_l, fast.pdf_g) == (res.index, res.score, res.pdf_l, res.pdf_g), \
            (case, dc, du, lev, n, scale, pair.good.has_neg, pair.bad.has_neg)
        if case % 10 == 0:
            l = O.pdf_many(X[g_idx], bwg, vt, C, nlg)
            g = O.pdf_many(X[b_idx], bwb, vt, C, nlb)
            assert fast.index == O.select(l, g)[0], case


def _capi_logpdf_rtol(k, C, rtol=1e-5):
    """hbx_kde_logpdf_rtol called straight through the C-ABI (what a reference-side integrator binds)."""
    import torch
    from hpbandster_amd import _native as N
    L = N.lib()
    C = np.ascontiguousarray(C, dtype=np.float64)
    c_dev = torch.from_numpy(C).to(k.device)
    out = torch.full((C.shape[0],), 123.0, dtype=torch.float64, device=k.device)
    sb = int(L.hbx_kde_logpdf_rtol_scratch_bytes(C.shape[0]))
    scr = torch.empty(sb, dtype=torch.uint8, device=k.device)
    N.call("hbx_kde_logpdf_rtol", N.ptr(c_dev), C.shape[0], C.shape[1], N.ptr(k.params), N.ptr(k.table),
           N.ptr(k.X_dev), N.ptr(k.rows_dev), k.dc_pad, k.du_pad, k.variant, rtol, N.ptr(out), N.ptr(scr), sb,
           N.stream_handle(None, k.device))
    return out.cpu().numpy()


@pytest.mark.parametrize("lut", ["1", "0"])
@pytest.mark.parametrize("rtol", [1e-5, 1e-9])
@pytest.mark.parametrize("case", ["outlier", "d46", "signed", "d32m", "far24c8u", "cat_only"])
def test_capi_logpdf_rtol_contract(device, case, rtol, lut, monkeypatch):
    """The north-star ln-pdf contract at the C-ABI (not through DeviceKDE): within rtol * max(1, |ln p|)
    of the reference's ln pdf for every candidate where that is finite, NaN where it is NaN -- next to an
    outlying observation, at D = 46, on a KDE with negative categorical factors, and at config #3's shape.
    rtol 1e-5 (the north star's): the fp32 direct-difference pass writes the candidates its bound accepts;
    rtol 1e-9: its bound accepts none, and every candidate takes the fp64 pass (tiled kernel, fp64 exp2).
    lut: the direct-difference pass matches categorical codes through its LDS tables (HBX_DD_LUT=1, KDEs whose
    codes fit two bits) or through the packed compare (0)."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    monkeypatch.setenv("HBX_DD_LUT", lut)
    rs = np.random.RandomState(11)
    if case == "outlier":
        n, D = 8500, 16
        X = 0.5 + 1e-3 * rs.rand(n, D)
        X[17] = 0.0
        Lo = rs.rand(n)
        Lo[17] = np.sort(Lo)[n // 2]
        vt = "c" * D
        C = np.vstack([0.5 + 1e-3 * rs.rand(200, D), 0.02 * rs.rand(56, D)])
    elif case == "d46":
        dc, lv = 30, [4] * 16
        X = S.make_observations(2000, dc, 16, lv, seed=21)
        Lo = S.make_losses(2000, seed=22)
        vt = S.var_type_string(dc, 16)
        C = S.make_candidates(256, dc, 16, lv, seed=23)
    elif case == "signed":
        c = G.load_kde_case("hgt1")
        X, Lo, vt, C = c["X"], c["eff_losses"], c["var_type"], c["cands"]
    elif case == "far24c8u":  # config #3's dims, uniform candidates: every one re-evaluated in fp64
        X = S.make_observations(1500, 24, 8, 4, seed=24)
        Lo = S.make_losses(1500, seed=25)
        vt = S.var_type_string(24, 8)
        C = S.make_candidates(700, 24, 8, 4, seed=26)  # 2 full + 1 ragged block of the tiled kernel
        C[3, 5] = 40.0  # far outside the data
        C[9, 30] = 7.5  # a code no observation has
    elif case == "cat_only":
        X = S.make_observations(300, 0, 6, 5, seed=27)
        Lo = S.make_losses(300, seed=28)
        vt = S.var_type_string(0, 6)
        C = S.make_candidates(300, 0, 6, 5, seed=29)
    else:
        c = G.load_kde_case("d32m")
        X, Lo, vt, C = c["X"], c["eff_losses"], c["var_type"], c["cands"][:96]
    pair = kde.fit_pair(X, Lo, vt, len(vt) + 1, device=device)
    for k in (pair.good, pair.bad):
        lref = O.log_pdf_many(k.data, k.bw, vt, C, k.nlev)
        if k.has_neg:  # negative factors: ln of the reference's own (possibly negative) pdf
            with np.errstate(divide="ignore", invalid="ignore"):
                lref = np.log(O.pdf_many(k.data, k.bw, vt, C, k.nlev))
        got = _capi_logpdf_rtol(k, C, rtol=rtol)
        fin = np.isfinite(lref)
        assert fin.sum() > 0
        assert np.array_equal(np.isnan(got), np.isnan(lref)), case
        err = np.abs(got[fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        # the oracle's log-space restatement is itself ~1e-13 from the reference's fp64 value
        assert err.max() <= max(rtol, 2e-12), (case, err.max())


@pytest.mark.parametrize("sg", ["1", "0"])
@pytest.mark.parametrize("lut", ["1", "0"])
@pytest.mark.parametrize("du", [0, 4, 8])
def test_dd_pass_terms_far_above_the_first_chunk(device, du, lut, sg, monkeypatch):
    """Candidates that sit on an observation of a later chunk while every observation of chunk 0 is thousands of
    log2 units away: the group holding that observation overflows the first chunk's reference point, which moves
    up and the group is summed again; candidates with codes outside [0, 3] take the fp64 pass under the tables.
    Every ln pdf within the contract of the oracle's.  sg: 8256 candidates (their scratch holds the staged rows:
    the scalar-staged kernel) or the LDS-staged kernel (HBX_DD_SG=0)."""
    from hpbandster_amd import kde
    monkeypatch.setenv("HBX_DD_LUT", lut)
    monkeypatch.setenv("HBX_DD_SG", sg)
    rs = np.random.RandomState(41)
    n, dc = 700, 24
    vt = "c" * dc + "u" * du
    X = np.empty((n, dc + du))
    X[:, :dc] = rs.rand(n, dc)
    X[:64, :dc] = 0.95 + 0.01 * rs.rand(64, dc)  # chunk 0: one far cluster
    X[:, dc:] = rs.randint(0, 4, (n, du))
    C = X[rs.choice(np.arange(64, n), 96, replace=False)].copy()
    C[:8, :dc] += 1e-3 * rs.rand(8, dc)
    if du:
        C[8, dc] = 5.0  # a code no observation has (outside the tables' two bits)
    rows = np.arange(n)
    bw = np.r_[np.full(dc, 0.05), np.full(du, 0.3)]
    nlev = np.r_[np.zeros(dc), np.full(du, 4)].astype(np.int32)
    pair = kde.fit_pair_from_rows(X, rows, rows, vt, bw, bw, nlev, nlev, device=device)
    k = pair.good
    if du:
        assert (k.variant >> 8) & 1
    C = np.tile(C, (86, 1))  # 8256 rows (the SG kernel runs from 8192 candidates; 16 B of scratch each >= 704 x 28 floats)
    lref = O.log_pdf_many(X, bw, vt, C[:96], nlev)
    got = _capi_logpdf_rtol(k, C)
    assert np.array_equal(got, np.tile(got[:96], 86))
    got = got[:96]
    assert np.isfinite(lref).all()
    err = np.abs(got - lref) / np.maximum(1.0, np.abs(lref))
    assert err.max() <= 1e-5, err.max()


@pytest.mark.parametrize("shape", [(8, 0, 0), (4, 4, 3), (8, 8, 4), (16, 16, 5), (24, 0, 0), (16, 8, 2)])
def test_dd_scalar_staged_across_buckets(device, shape, monkeypatch):
    """The SG instance in the other dd buckets it is built for (rows of at most 32 floats: continuous-only,
    two-bit codes through the tables, wider codes through the packed compare): bit-identical to the
    LDS-staged kernel on 8192 candidates, within the contract of the oracle on a sample."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du, lv = shape
    n = 900
    X = S.make_observations(n, dc, du, lv, seed=61 + dc + du)
    Lo = S.make_losses(n, seed=62)
    vt = S.var_type_string(dc, du)
    rs = np.random.RandomState(63)
    C = S.make_candidates(8192, dc, du, lv, seed=64)
    C[:3000] = X[rs.randint(0, n, 3000)]
    if dc:
        C[:3000, :dc] += 0.02 * rs.randn(3000, dc)
    pair = kde.fit_pair(X, Lo, vt, len(vt) + 1, device=device)
    sel = np.r_[np.arange(0, 8192, 160), 1, 2]
    for k in (pair.good, pair.bad):
        monkeypatch.setenv("HBX_DD_SG", "1")
        a = _capi_logpdf_rtol(k, C)
        monkeypatch.setenv("HBX_DD_SG", "0")
        b = _capi_logpdf_rtol(k, C)
        assert np.array_equal(a, b, equal_nan=True), shape
        lref = O.log_pdf_many(k.data, k.bw, vt, C[sel], k.nlev)
        if k.has_neg:
            with np.errstate(divide="ignore", invalid="ignore"):
                lref = np.log(O.pdf_many(k.data, k.bw, vt, C[sel], k.nlev))
        assert np.array_equal(np.isnan(a[sel]), np.isnan(lref)), shape
        fin = np.isfinite(lref)
        err = np.abs(a[sel][fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.max() <= 1e-5, (shape, err.max())


@pytest.mark.parametrize("lut", ["1", "0"])
def test_dd_scalar_staged_equals_lds_staged(device, lut, monkeypatch):
    """The scalar-staged direct-difference kernel (rows staged once into the call's scratch, read through SGPRs)
    against the LDS-staged one at config #3's dims (24c + 8u, 4 levels; 3000 observations, 20000 candidates:
    uniform draws, observations' neighbours, an unseen code, a far point): the same fp32 values in the same
    order, so the ln pdfs are equal bit for bit, and within 1e-5 of the oracle's on a sample (the good KDE's
    categorical bandwidths exceed 1 here: ln of the reference's signed pdf, NaN where that is negative)."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    monkeypatch.setenv("HBX_DD_LUT", lut)
    X = S.make_observations(3000, 24, 8, 4, seed=51)
    Lo = S.make_losses(3000, seed=52)
    vt = S.var_type_string(24, 8)
    rs = np.random.RandomState(53)
    C = S.make_candidates(20000, 24, 8, 4, seed=54)
    C[:5000] = X[rs.randint(0, 3000, 5000)]
    C[:5000, :24] += 0.01 * rs.randn(5000, 24)
    C[7, 30] = 7.0
    C[11, 2] = 30.0
    pair = kde.fit_pair(X, Lo, vt, 33, device=device)
    for k in (pair.good, pair.bad):
        monkeypatch.setenv("HBX_DD_SG", "1")
        a = _capi_logpdf_rtol(k, C)
        monkeypatch.setenv("HBX_DD_SG", "0")
        b = _capi_logpdf_rtol(k, C)
        assert np.array_equal(a, b, equal_nan=True)
        sel = np.r_[np.arange(0, 20000, 40), 7, 11]
        lref = O.log_pdf_many(k.data, k.bw, vt, C[sel], k.nlev)
        if k.has_neg:  # a categorical bandwidth above 1: ln of the reference's own (possibly negative) pdf
            with np.errstate(divide="ignore", invalid="ignore"):
                lref = np.log(O.pdf_many(k.data, k.bw, vt, C[sel], k.nlev))
        assert np.array_equal(np.isnan(a[sel]), np.isnan(lref))
        fin = np.isfinite(lref)
        assert fin.sum() > 100
        err = np.abs(a[sel][fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.max() <= 1e-5, err.max()


def test_dd_pass_no_finite_term_in_first_chunk(device):
    """A categorical bandwidth of exactly 1 (the Aitchison-Aitken match factor 1 - h is 0) with the first 64
    observations all matching the candidates in that dim: chunk 0 of the direct-difference pass has no finite
    term, so its reference point is not a term of the sum and the bound does not hold; those candidates take the
    fp64 pass, and every ln pdf meets the contract."""
    from hpbandster_amd import kde
    rs = np.random.RandomState(31)
    n, dc = 400, 8
    vt = "c" * dc + "uu"
    X = np.empty((n, dc + 2))
    X[:, :dc] = rs.rand(n, dc)
    X[:64, dc] = 1.0                             # chunk 0: every row matches the candidates' code 1 ...
    X[64:, dc] = 2.0 * rs.randint(0, 2, n - 64)  # ... and no later row does
    X[:, dc + 1] = rs.randint(0, 3, n)
    C = rs.rand(96, dc + 2)
    C[:, dc] = 1.0
    C[:, dc + 1] = rs.randint(0, 3, 96)
    rows = np.arange(n)
    bw = np.r_[np.full(dc, 0.2), 1.0, 0.3]
    nlev = np.r_[np.zeros(dc, dtype=np.int32), 3, 3].astype(np.int32)
    pair = kde.fit_pair_from_rows(X, rows, rows, vt, bw, bw, nlev, nlev, device=device)
    k = pair.good
    lref = O.log_pdf_many(X, bw, vt, C, nlev)
    for rtol in (1e-5, 1e-7):
        got = _capi_logpdf_rtol(k, C, rtol=rtol)
        fin = np.isfinite(lref)
        assert fin.all()
        err = np.abs(got - lref) / np.maximum(1.0, np.abs(lref))
        assert err.max() <= max(rtol, 2e-12), (rtol, err.max())


@pytest.mark.parametrize("dc,du,lev", [(24, 8, 4), (8, 0, 2), (16, 4, 3), (32, 4, 2)])
def test_coarse_prescreen_matches_fast_and_oracle(device, dc, du, lev, monkeypatch):
    """The acquisition's coarse pre-screen (one f16 product per continuous dim, the dropped products in
    each candidate's bound; variant bit 7) against the FAST instance (HBX_COARSE=0: three products per
    dim) and the oracle: the same record (index, score, pdfs) at config #3's dims and others; the exact
    re-score takes a few more candidates."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    n = 3000
    X = S.make_observations(n, dc, du, lev, seed=81)
    L = S.make_losses(n, seed=82)
    vt = S.var_type_string(dc, du)
    C = S.make_candidates(5000, dc, du, lev, seed=83)
    monkeypatch.setenv("HBX_COARSE", "1")
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    for k in (pair.good, pair.bad):  # every unsigned h32 KDE carries the coarse table
        assert (k.variant >> 7) & 1 == (0 if k.has_neg else 1)
    assert not pair.bad.has_neg
    co = pair.acquire(C)
    monkeypatch.setenv("HBX_COARSE", "0")
    pair0 = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    assert (pair0.bad.variant >> 7) & 1 == 0
    fa = pair0.acquire(C)
    assert (co.index, co.score, co.pdf_l, co.pdf_g) == (fa.index, fa.score, fa.pdf_l, fa.pdf_g)
    assert co.shortlist >= fa.shortlist >= 1
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C[:800], pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C[:800], pair.bad.nlev)
    assert pair.acquire(C[:800]).index == O.select(l, g)[0]


@pytest.mark.parametrize("nc", [1, 31, 32, 33, 63, 64, 65, 100, 511, 512, 513, 577])
def test_coarse_two_column_tiles_ragged(device, nc, monkeypatch):
    """The coarse instance's waves hold 64 candidates (two 32-column tiles): candidate counts that end inside
    the first or the second column tile of a wave, or of a 512-candidate block, give the FAST instance's
    record; and with the oracle's best candidate moved to the LAST position (column tile 1 of the last wave
    when nc mod 64 > 32) the pick follows it."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du, lev, n = 24, 8, 4, 2000
    X = S.make_observations(n, dc, du, lev, seed=91)
    L = S.make_losses(n, seed=92)
    vt = S.var_type_string(dc, du)
    C = S.make_candidates(max(nc, 2), dc, du, lev, seed=93)[:nc].copy()
    monkeypatch.setenv("HBX_COARSE", "1")
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    assert (pair.bad.variant >> 7) & 1 == 1
    monkeypatch.setenv("HBX_COARSE", "0")
    pair0 = kde.fit_pair(X, L, vt, dc + du + 1, device=device)
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    best = O.select(l, g)[0]
    order = [i for i in range(nc) if i != best] + [best]
    for cands, want in ((C, best), (C[order], nc - 1)):
        co, fa = pair.acquire(cands), pair0.acquire(cands)
        assert (co.index, co.score, co.pdf_l, co.pdf_g) == (fa.index, fa.score, fa.pdf_l, fa.pdf_g)
        assert co.index == want


@pytest.mark.parametrize("dc,du,nobs,nc,far", [(24, 8, 3000, 512, True), (24, 8, 10000, 4099, False),
                                               (16, 0, 700, 1, False), (16, 4, 1500, 513, True),
                                               (8, 12, 2000, 1025, False), (32, 4, 900, 2048, True)])
def test_acquire_reused_workspace_and_ragged_tiles(device, dc, du, nobs, nc, far):
    """One workspace reused across acquisitions (over other candidates in between) gives the records of
    fresh workspaces field by field, at every tile fill, with rescue markers (far candidates); the winner
    is the oracle's."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(dc, du)
    X = S.make_observations(nobs, dc, du, 4, seed=71 + dc)
    L = S.make_losses(nobs, seed=72 + du)
    C = S.make_candidates(nc, dc, du, 4, seed=73 + nc)
    if far:
        C[min(5, nc - 1), 0] = 1000.0
        C[nc // 2, dc - 1] = -400.0
    pair = kde.fit_pair(X, L, vt, dc + du + 1, device=device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g, r.shortlist, r.flags, r.near, r.rel)
    ref = rec(pair.acquire(C))
    C2 = C[::-1].copy()
    ref2 = rec(pair.acquire(C2))
    ws = torch.full((pair.workspace_bytes(nc),), 0xA5, dtype=torch.uint8, device=device)
    for rep in range(2):
        assert rec(pair.acquire(C, workspace=ws)) == ref, rep
        assert rec(pair.acquire(C2, workspace=ws)) == ref2, rep
    if nc * nobs > 4e6:
        return
    l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
    g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    assert ref[0] == O.select(l, g)[0]


@pytest.mark.parametrize("nc", [300, 2500])
def test_large_shortlists_through_the_synchronous_call(device, nc):
    """The drop-in's synchronous call (hbx_kde_acquire_bound: the record published to mapped memory without a
    system fence) at shortlists past the in-LDS 256 (300) and past the split cap (2500: one work item per
    candidate, all units in turn) picks the C oracle's candidate with its pdfs; repeated on one workspace,
    forward and reversed (the previous call's state and record must not leak)."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    from oracle import c_oracle
    dc = 70
    X = S.make_observations(320, dc, 0, 0, seed=81)
    vt = S.var_type_string(dc, 0)
    pair = kde.fit_pair(X, S.make_losses(320, seed=82), vt, dc + 1, device=device)
    assert pair.good.exact_only  # every candidate re-scored: the shortlist is the whole set
    C = S.make_candidates(nc, dc, 0, 0, seed=83)
    C[:40] = X[pair.good.rows_dev.cpu().numpy()[:40]] + 1e-3
    Cd = torch.from_numpy(C).to(device)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g, r.shortlist, r.flags, r.near, r.rel)
    first = rec(pair.acquire(Cd, workspace=ws))
    for _ in range(3):
        back = pair.acquire(torch.flip(Cd, [0]).contiguous(), workspace=ws)
        assert back.score == first[1] and back.shortlist == nc
        assert rec(pair.acquire(Cd, workspace=ws)) == first
    assert first[4] == nc
    l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
    g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    want, _ = O.select(l, g)
    assert first[0] == want and (first[2], first[3]) == (l[want], g[want])


@pytest.mark.parametrize("nc,nobs,far", [(64, 10000, False), (64, 10000, True), (700, 4000, False), (5000, 3000, True)])
def test_observation_splits_pick_like_one_range(device, monkeypatch, nc, nobs, far):
    """Few candidates against many observations: the scoring blocks split the observations into chunk
    ranges whose partial estimates the combine kernel merges (HBX_OBS_SPLIT=1, the default) -- the exact
    pick, its score and both pdfs equal the unsplit launch's, with rescue markers in some ranges (far
    candidates) too; and the winner is the oracle's."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    X = S.make_observations(nobs, 24, 8, 4, seed=91)
    vt = S.var_type_string(24, 8)
    pair = kde.fit_pair(X, S.make_losses(nobs, seed=92), vt, 33, device=device)
    C = S.make_candidates(nc, 24, 8, 4, seed=93)
    if far:
        C[3, 0] = 900.0
        C[nc // 2, 5] = -300.0
    Cd = torch.from_numpy(C).to(device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g)
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")
    one = pair.acquire(Cd)
    monkeypatch.setenv("HBX_OBS_SPLIT", "1")
    for _ in range(2):
        assert rec(pair.acquire(Cd)) == rec(one)
    rb = pair.acquire_batch(Cd, max(1, nc // 4))
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")
    rb0 = pair.acquire_batch(Cd, max(1, nc // 4))
    assert [rec(a) for a in rb] == [rec(b) for b in rb0]
    if nc * nobs <= 1e6:
        l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
        g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
        assert one.index == O.select(l, g)[0]


@pytest.mark.parametrize("nobs,far", [(4000, False), (10000, True)])
def test_observation_splits_signed_kdes(device, monkeypatch, nobs, far):
    """Both KDEs signed (categorical bandwidths above 1: every factor 1 - h < 0, so partial sums of either
    sign) and enough observations for both to split (>= 8 chunks each) at 64 candidates: the merged partial
    estimates give the unsplit launch's record (index, score, pdfs), single and batched, and the oracle's
    winner."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du = 24, 8
    vt = S.var_type_string(dc, du)
    X = S.make_observations(nobs, dc, du, 4, seed=97)
    g_idx, b_idx = O.bohb_split(X, S.make_losses(nobs, seed=98), dc + du + 1)
    assert len(g_idx) >= 8 * 64 and len(b_idx) >= 8 * 64
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    bwg[dc:], bwb[dc:] = 1.25, 1.4
    nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, nlg, nlb)
    assert pair.good.has_neg and pair.bad.has_neg
    C = S.make_candidates(64, dc, du, 4, seed=99)
    C[::2, dc:] = X[g_idx[:32], dc:]  # half the candidates on a good row's levels
    if far:
        C[7, 2] = 800.0
    Cd = torch.from_numpy(C).to(device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g)
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")
    one = pair.acquire(Cd)
    rb0 = pair.acquire_batch(Cd, 16)
    monkeypatch.setenv("HBX_OBS_SPLIT", "1")
    for _ in range(2):
        assert rec(pair.acquire(Cd)) == rec(one)
    assert [rec(a) for a in pair.acquire_batch(Cd, 16)] == [rec(b) for b in rb0]
    l = O.pdf_many(X[g_idx], bwg, vt, C, nlg)
    g = O.pdf_many(X[b_idx], bwb, vt, C, nlb)
    assert one.index == O.select(l, g)[0]


@pytest.mark.parametrize("nc,nobs", [(512, 3000), (64, 300), (2100, 1500)])
def test_rescue_in_the_combine_kernel_equals_its_own_launch(device, monkeypatch, nc, nobs):
    """A single acquisition scored by the 32x32 pair kernel leaves the rescue pass to the combine kernel
    (one launch less; a copy of the rescue arithmetic without register arrays).  With far candidates
    (markers in both KDEs) its record equals, field by field, the record of the same candidates as one
    segment of a batched acquisition (which runs the separate rescue launch), and its ln-pdf estimates equal
    those of two single-KDE launches (HBX_SCORE_PAIR=0, whose rescue is a launch of its own) bit for bit; the
    winner is the oracle's."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(nobs, 24, 8, 4, seed=101)
    pair = kde.fit_pair(X, S.make_losses(nobs, seed=102), vt, 33, device=device)
    assert (pair.good.variant >> 6) & 1 and (pair.bad.variant >> 6) & 1
    C = S.make_candidates(nc, 24, 8, 4, seed=103)
    C[min(5, nc - 1), 0] = 1000.0
    C[nc // 2, 3] = -400.0
    C[nc - 1, 23] = 2500.0
    Cd = torch.from_numpy(C).to(device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g, r.shortlist, r.flags, r.near, r.rel)

    def run():
        res, logl, logg = pair.acquire(Cd, logs=True)
        return rec(res), np.asarray(logl).tobytes(), np.asarray(logg).tobytes(), rec(pair.acquire(Cd))
    inline = run()
    assert rec(pair.acquire_batch(Cd, nc)[0]) == inline[3]
    monkeypatch.setenv("HBX_SCORE_PAIR", "0")
    assert run()[:3] == inline[:3]
    monkeypatch.delenv("HBX_SCORE_PAIR")
    lref = O.log_pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
    assert np.isfinite(lref[[min(5, nc - 1), nc // 2, nc - 1]]).sum() >= 2  # far, yet finite: rescued
    if nc * nobs <= 2e6:
        l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
        g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
        assert inline[0][0] == O.select(l, g)[0]


@pytest.mark.parametrize("case", ["mixed", "exact_only", "far", "one", "full"])
def test_exact_scan_equals_the_shortlist_launch(device, monkeypatch, case):
    """A single acquisition of <= 1024 candidates has no shortlist launch: every exact re-score block
    shortlists for itself (the shortlist kernel's predicate in index order).  Its record equals field by
    field that of the same candidates as one segment of a batched acquisition (the shortlist launch) --
    every candidate re-scored (exact_only), rescue markers (far), one candidate, the 1024 cap -- repeated
    calls on one workspace agree, and the winner is the oracle's."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du, nobs, nc = {"mixed": (24, 8, 3000, 64), "exact_only": (70, 0, 320, 300), "far": (16, 4, 1500, 513),
                        "one": (8, 4, 900, 1), "full": (8, 12, 2000, 1024)}[case]
    vt = S.var_type_string(dc, du)
    X = S.make_observations(nobs, dc, du, 4 if du else 0, seed=111 + dc)
    pair = kde.fit_pair(X, S.make_losses(nobs, seed=112), vt, dc + du + 1, device=device)
    C = S.make_candidates(nc, dc, du, 4 if du else 0, seed=113 + nc)
    if case == "far":
        C[5, 0] = 1000.0
        C[nc // 2, dc - 1] = -400.0
    if case == "exact_only":
        assert pair.good.exact_only
        C[:20] = X[pair.good.rows_dev.cpu().numpy()[:20]] + 1e-3
    Cd = torch.from_numpy(C).to(device)

    def rec(r):
        return (r.index, r.score, r.pdf_l, r.pdf_g, r.shortlist, r.flags, r.near, r.rel)

    def run():
        res, logl, logg = pair.acquire(Cd, logs=True)
        return rec(res), np.asarray(logl).tobytes(), np.asarray(logg).tobytes(), rec(pair.acquire(Cd))
    scan = run()
    assert rec(pair.acquire_batch(Cd, nc)[0]) == scan[3]
    assert run() == scan  # the workspace after a shortlist launch
    if nc * nobs <= 2e6:
        l = O.pdf_many(pair.good.data, pair.good.bw, vt, C, pair.good.nlev)
        g = O.pdf_many(pair.bad.data, pair.bad.bw, vt, C, pair.bad.nlev)
        assert scan[0][0] == O.select(l, g)[0]


@pytest.mark.parametrize("case", range(10))
def test_dd_scalar_staged_random_shapes(device, case, monkeypatch):
    """Seeded random shapes for the SG instance (continuous and categorical counts, level counts, observation
    counts that are not multiples of the group size or of a chunk, fewer than one chunk): bit-identical to the
    LDS-staged kernel on >= 8192 candidates, within the contract of the oracle on a sample."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    rs = np.random.RandomState(700 + case)
    dc = int(rs.randint(1, 29))
    du = int(rs.randint(0, 9))
    lv = int(rs.randint(2, 7))
    n = int(rs.choice([40, 63, 65, 131, 517, 1003, 2999]))
    nc = 8192 + int(rs.randint(0, 700))
    X = S.make_observations(n, dc, du, lv, seed=800 + case)
    Lo = S.make_losses(n, seed=900 + case)
    vt = S.var_type_string(dc, du)
    C = S.make_candidates(nc, dc, du, lv, seed=1000 + case)
    C[: nc // 3] = X[rs.randint(0, n, nc // 3)]
    C[: nc // 3, :dc] += 0.02 * rs.randn(nc // 3, dc)
    pair = kde.fit_pair(X, Lo, vt, min(len(vt) + 1, n - 1), device=device)
    assert pair is not None, (dc, du, n)
    sel = np.r_[np.arange(0, nc, 97), 0, 1]
    for k in (pair.good, pair.bad):
        monkeypatch.setenv("HBX_DD_SG", "1")
        a = _capi_logpdf_rtol(k, C)
        monkeypatch.setenv("HBX_DD_SG", "0")
        b = _capi_logpdf_rtol(k, C)
        assert np.array_equal(a, b, equal_nan=True), (dc, du, lv, n)
        lref = O.log_pdf_many(k.data, k.bw, vt, C[sel], k.nlev)
        if k.has_neg:
            with np.errstate(divide="ignore", invalid="ignore"):
                lref = np.log(O.pdf_many(k.data, k.bw, vt, C[sel], k.nlev))
        assert np.array_equal(np.isnan(a[sel]), np.isnan(lref)), (dc, du, lv, n)
        fin = np.isfinite(lref)
        err = np.abs(a[sel][fin] - lref[fin]) / np.maximum(1.0, np.abs(lref[fin]))
        assert err.size == 0 or err.max() <= 1e-5, ((dc, du, lv, n), err.max())


@pytest.mark.parametrize("nc,dc,du,n", [(100000, 8, 0, 1000), (20000, 24, 8, 3000), (700, 16, 0, 500),
                                        (64, 24, 8, 10000), (131072, 8, 0, 1000)])
def test_one_tile_pair_kernel_same_records(device, nc, dc, du, n, monkeypatch):
    """Launches whose two KDEs' blocks fit one round of the chip's slots take the coarse pair kernel with one
    candidate column tile per wave (kde_logpdf_h32_pair1_kernel); HBX_PAIR1=0 keeps the two-tile kernel.  Same
    record either way (index, score, shortlist, near, flags) -- the winner the C oracle's."""
    from oracle import c_oracle
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    X = S.make_observations(n, dc, du, 4)
    vt = S.var_type_string(dc, du)
    pair = kde.fit_pair(X, S.make_losses(n), vt, dc + du + 1, device=device)
    C = S.make_candidates(nc, dc, du, 4, seed=9)
    recs = []
    for v in ("1", "0"):
        monkeypatch.setenv("HBX_PAIR1", v)
        r = pair.acquire(C)
        recs.append((r.index, r.score, r.shortlist, r.near, r.flags, r.pdf_l, r.pdf_g))
    assert recs[0] == recs[1]
    if nc <= 20000:
        l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
        assert recs[0][0] == O.select(l, g)[0]
