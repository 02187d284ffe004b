"""Grouped cv_ml bandwidths (hbx_kde_cv_groups): the objective against a plain fp64 numpy form, the selection against
statsmodels' committed answers and against scipy.optimize.fmin over that numpy form, and the wiring."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52


def ref_terms(X, vt, h):
    """ln L_i of every row (leave-one-out, one exponential per pair, the normaliser in log space) and, per row, the
    term-weighted mean of (|exponent| + dc + du + 4): the relative error bound of L_i in units of 2^-52."""
    cont = np.array([t == "c" for t in vt])
    T = X[:, None, cont] - X[None, :, cont]
    E = (T * T * (1.0 / (2.0 * h[cont] ** 2))).sum(-1)
    P = np.exp(-E)
    for d in np.nonzero(~cont)[0]:
        _, inv, cnt = np.unique(X[:, d], return_inverse=True, return_counts=True)
        c = cnt.size - (cnt[inv] == 1)  # the level count of the column without row i
        P = P * np.where(X[:, None, d] == X[None, :, d], 1.0 - h[d], (h[d] / (c - 1.0))[:, None])
    np.fill_diagonal(P, 0.0)
    L = P.sum(1)
    units = (P * (E + len(vt) + 4)).sum(1) / L
    return np.log(L) - np.log(h[cont]).sum() - 0.5 * cont.sum() * np.log(2 * np.pi), L, units


def ref_objective(X, vt, h):
    with np.errstate(all="ignore"):
        return -ref_terms(X, vt, np.asarray(h, dtype=np.float64))[0].sum()


def ref_select(X, vt, h0):
    """statsmodels' cv_ml selection over ref_objective: fmin as SM:_kernel_base.py:326-327 calls it, then the bounds"""
    from scipy import optimize
    bw = optimize.fmin(lambda h: ref_objective(X, vt, h), x0=h0, maxiter=1e3, maxfun=1e3, disp=0, xtol=1e-3)
    bw[bw < 0] = 1e-10
    cat = np.array([t == "u" for t in vt])
    bw[cat] = np.minimum(bw[cat], 1.0)
    return bw


def make_groups(seed, vt, lens, const_col_group=None, single=True):
    """Ragged groups: uniform continuous columns, codes 0..2 in the categorical ones and (``single``) one row per
    group at a level of its own (a level that occurs once: the leave-one-out level count); losses without ties."""
    rs = np.random.RandomState(seed)
    N, D = int(np.sum(lens)), len(vt)
    X = rs.rand(N, D)
    seg = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    for d, t in enumerate(vt):
        if t == "u":
            X[:, d] = rs.randint(0, 3, N)
            if single:
                X[seg[:-1][np.asarray(lens) > 0] + (d % 2), d] = 7.0
    if const_col_group is not None:
        X[seg[const_col_group]:seg[const_col_group + 1], 0] = 0.25
    return X, rs.permutation(N).astype(np.float64), seg


def kde_rows(gm, X, b):
    s = int(gm.seg_host[b])
    return [X[s + r] for r in gm.rows_of(b)]


@pytest.mark.gpu
@pytest.mark.parametrize("vt", ["c", "cuc", "ccuccuccc", "ccucccuccucccuccu"])
def test_objective_against_numpy(device, vt):
    """HBX_CV_EVAL against ref_terms at the normal-reference bandwidths and at 0.2 and 5 times them (categorical ones
    kept below 1 so that every term is positive), for KDEs of D + 1 rows, of 65 rows (one past an LDS chunk), of 263
    rows (a second pass over the block's 256 lanes) and a group without a model.

    Bound on |f - f_ref|, in units of 2^-52: a term exp(-e) prod_u a_u carries (|e| + dc + du + 4) -- the
    exponent's rounding amplified by |e|, one ulp per factor and for exp --, positive terms keep the term-weighted
    mean of that through the sum over j (ref_terms' ``units``), ln adds one ulp of |ln L_i| and the sum over i at most
    n ulps of sum_i |ln L_i|: sum_i units_i + (1 + n) sum_i |ln L_i|; twice that, since the reference rounds too."""
    from hpbandster_amd import groups
    D = len(vt)
    lens = [D + 1, 77, D, 310]
    X, losses, seg = make_groups(11, vt, lens)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    assert list(gm.has_model) == [True, True, False, True] and gm.n_bad[1] == 65 and gm.n_bad[3] == 263
    cat = np.array([t == "u" for t in vt])
    for scale in (1.0, 0.2, 5.0):
        bws = [np.where(cat, np.minimum(bw * scale, 0.95), bw * scale) for bw in gm.bandwidths()]
        got = gm.cv_objective(bws[0], bws[1]).cpu().numpy()
        assert got.shape == (4, 2) and np.isnan(got[2]).all()
        for b in (0, 1, 3):
            for side, rows in enumerate(kde_rows(gm, X, b)):
                ln_l, L, units = ref_terms(rows, vt, bws[side][b])
                assert (L > 0).all()
                bound = 2 * EPS * (units.sum() + (1 + len(rows)) * np.abs(ln_l).sum())
                err = abs(got[b, side] + ln_l.sum())
                print(vt, scale, b, side, len(rows), "err %.3g bound %.3g" % (err, bound))
                assert err <= bound, (vt, scale, b, side, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name,evals", [("cv_c3", 93), ("cv_c6", 265), ("cv_mixed", 118)])
def test_selection_against_statsmodels(device, name, evals):
    """The device search on statsmodels' own inputs: its committed cv_ml selection within the project's tolerance
    for CV selections, converged, after as many evaluations as scipy makes on the plain objective."""
    from hpbandster_amd import cv, groups
    g = np.load(os.path.join(GOLD, name + ".npz"))
    X, vt = g["X"], str(g["var_type"])
    np.testing.assert_allclose(cv.select_bandwidth(X, vt, "cv_ml", device=device, search="device"), g["bw_cv_ml"],
                               rtol=1e-6)
    info = {}
    cv.select_cv_ml_device(X, vt, device=device, info=info)
    print(name, info)
    assert info["status"] == groups.CV_CONVERGED and info["evals"] == evals


CASES = {  # var_type, group lengths, seed, fit_groups keywords, the group with a constant column
    "cc": ("cc", [14, 40, 2, 25], 3, {}, None),
    "ccuu": ("ccuu", [60, 4, 90, 45], 2, {}, None),
    "min_bw": ("cuc", [40, 70], 8, dict(min_bandwidth=0.3), None),
    "const": ("cc", [18, 30], 9, {}, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_search_against_fmin(device, case):
    """fit_groups(bw='cv_ml') against scipy.optimize.fmin over ref_objective from the same normal-reference start:
    the bounds and min_bandwidth applied, groups without a model skipped, a constant column left at its
    normal-reference bandwidths, and two runs byte for byte the same."""
    from hpbandster_amd import groups
    vt, lens, seed, kw, const = CASES[case]
    X, losses, seg = make_groups(seed, vt, lens, const, single=False)
    nr = groups.fit_groups(X, losses, seg, vt, device=device, **kw)  # the search's start: the fit's bandwidths
    gm = groups.fit_groups(X, losses, seg, vt, device=device, bw="cv_ml", **kw)
    again = groups.fit_groups(X, losses, seg, vt, device=device, bw="cv_ml", **kw)
    status, evals = gm.bw_status.cpu().numpy(), gm.bw_evals.cpu().numpy()
    for a, b in zip(gm.bandwidths() + (gm.bw_objective.cpu().numpy(), status, evals),
                    again.bandwidths() + (again.bw_objective.cpu().numpy(), again.bw_status.cpu().numpy(),
                                          again.bw_evals.cpu().numpy())):
        assert a.tobytes() == b.tobytes()
    for b in range(len(lens)):
        if not gm.has_model[b]:
            assert (status[b] == groups.CV_NO_MODEL).all() and np.isnan(gm.bandwidths()[0][b]).all()
            continue
        for side, rows in enumerate(kde_rows(nr, X, b)):
            h0, got = nr.bandwidths()[side][b], gm.bandwidths()[side][b]
            if b == const:
                assert status[b, side] == groups.CV_NOT_SEARCHABLE and evals[b, side] == 0
                assert got.tobytes() == h0.tobytes()
                continue
            want = np.maximum(ref_select(rows, vt, h0), kw.get("min_bandwidth", 0.0))
            print(case, b, side, status[b, side], evals[b, side], got, want)
            assert status[b, side] == groups.CV_CONVERGED
            np.testing.assert_allclose(got, want, rtol=1e-6)
            f = gm.bw_objective.cpu().numpy()[b, side]
            assert np.isfinite(f) and f <= ref_objective(rows, vt, h0)


@pytest.mark.gpu
def test_group_bohb_uses_the_rule(device):
    """GroupBOHB(bw_estimation='cv_ml'): the refit's bandwidths are fit_groups(bw='cv_ml')'s on the same rows, and
    get_configs answers from that model."""
    from hpbandster_amd import groups
    B, m, vt = 3, 24, "ccu"
    rs = np.random.RandomState(2)
    X = rs.rand(B, m, 3)
    X[:, :, 2] = rs.randint(0, 3, (B, m))
    losses = rs.rand(B, m)
    opt = groups.GroupBOHB(B, vt, [0, 0, 3], seed=1, device=device, bw_estimation="cv_ml")
    assert opt.new_results(1.0, X, losses)
    gm = groups.fit_groups(X.reshape(B * m, 3), losses.reshape(-1), np.arange(B + 1) * m, vt, 4, device=device,
                           bw="cv_ml")
    got = opt.kde_models[1.0]
    assert (got.bw_status.cpu().numpy() <= groups.CV_LIMIT).all() and (got.bw_evals.cpu().numpy() > 3).all()
    for a, b in zip(got.bandwidths(), gm.bandwidths()):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(gm.bandwidths()[0], groups.fit_groups(
        X.reshape(B * m, 3), losses.reshape(-1), np.arange(B + 1) * m, vt, 4, device=device).bandwidths()[0])
    cfg = opt.get_configs(1.0, S=8)
    assert cfg.rows.shape == (B, 8, 3) and cfg.model_based.any() and np.isfinite(cfg.rows).all()
