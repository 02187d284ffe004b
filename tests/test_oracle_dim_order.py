"""The oracle pinned for mixed column orders (no GPU).

tests/test_oracle_golden.py pins oracle/kde_oracle.c and oracle/kde_oracle.py against reference outputs that are all
continuous-first.  Here every case the GPU tests of tests/test_gpu_dim_order*.py use (tests/dim_orders.py builds them
for both files) is evaluated twice, on the permuted data and on the c-first arrangement of the same data, and

(a) the C oracle's exact pdfs agree within dim_orders.pdf_bound: the per-dim kernel factors are bit-identical in both
    arrangements, only the D - 1 products, the dc - 1 products of prod(bw[continuous]), the division and the pairwise
    sum round differently -- a bandwidth, level count or coordinate taken from the wrong dim misses it by orders of
    magnitude.  Signed KDEs (a factor 1 - h < 0) get the same bound relative to the sum of the terms' magnitudes;
(b) the numpy transcription kde_oracle.pdf_many agrees with the C oracle on the permuted data within that bound plus
    4 ulp per continuous dim (this numpy's exp is not the 1.26.4 one the C oracle restates);
(c) the order matters: at D >= 8 at least one candidate in ten has other pdf bits in the two arrangements, so a
    bit-for-bit pass on the GPU says something about the order of the products;
(d) kde_oracle.log_pdf_many and kde_oracle.cv_terms pass the permutation check too, with bounds derived below.
"""
import math

import numpy as np
import pytest

from oracle import c_oracle
from oracle import kde_oracle as O
from tests import dim_orders as DO

EPS = DO.EPS
TINY = 1e-290  # below it the pdfs approach the subnormals, where a relative bound does not hold


def _abs_pdf(data, bw, vt, nlev, pts):
    """sum_i prod_d |K_d(i)| / prod(bw[c]) / n: the magnitude a signed sum's rounding errors are relative to"""
    out = np.empty(len(pts))
    iscont = np.array([t == "c" for t in vt])
    with np.errstate(all="ignore"):
        for j, x in enumerate(pts):
            K = np.empty(data.shape)
            for d, t in enumerate(vt):
                K[:, d] = O._gaussian(bw[d], data[:, d], x[d]) if t == "c" else \
                    np.abs(O._aitchison_aitken(bw[d], data[:, d], x[d], np.asarray(nlev[d])))
            out[j] = (K.prod(axis=1) / np.prod(bw[iscont])).sum() / data.shape[0]
    return out


def _check_perm(p, p0, bound, where, scale=None):
    """pdfs p (permuted) and p0 (c-first) of the same candidates: NaN and inf at the same places, and within bound
    (relative to p0, or to ``scale`` for signed sums) wherever p0 is above TINY.  Returns the worst ratio."""
    assert np.array_equal(np.isnan(p), np.isnan(p0)), where
    inf = np.isinf(p0)
    assert np.array_equal(p[inf], p0[inf]), where
    ref = np.abs(p0) if scale is None else scale
    ok = np.isfinite(p0) & (ref > TINY)
    assert ok.sum() >= 20, (where, int(ok.sum()))
    ratio = float((np.abs(p[ok] - p0[ok]) / ref[ok]).max()) / bound
    assert ratio <= 1.0, (where, ratio)
    return ratio


def _signed(bw, vt):
    return any(t == "u" and h > 1.0 for t, h in zip(vt, bw))


# ---- (a), (b), (c): the single-pair cases --------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", DO.pair_case_ids())
def test_pair_cases_permutation_invariant(name, order):
    c = DO.pair_case(name, order)
    assert c.vt != c.vt0 and sorted(c.vt) == sorted(c.vt0)
    worst = 0.0
    for which, (data, bw, nlev, data0, bw0, nlev0, p, p0) in zip("lg", c.kdes()):
        bound = DO.pdf_bound(c.D, c.dc, len(data))
        if _signed(bw, c.vt):
            m = 128  # the magnitudes come from numpy, one candidate at a time
            scale = _abs_pdf(data, bw, c.vt, nlev, c.C[:m])
            worst = max(worst, _check_perm(p[:m], p0[:m], bound, (name, order, which, "signed"), scale=scale))
            continue
        worst = max(worst, _check_perm(p, p0, bound, (name, order, which)))
        # (b) the numpy transcription on the permuted data
        m = 96
        with np.errstate(all="ignore"):
            q = O.pdf_many(data, bw, c.vt, c.C[:m], nlev)
        _check_perm(q, p[:m], bound + 4 * c.dc * 2 * EPS, (name, order, which, "pdf_many"))
    share = c.order_sensitive_share()
    print("%s %s %s: worst ratio to the bound %.3f, order-sensitive share %.2f" % (name, order, c.vt, worst, share))
    if c.D >= 8:
        assert share >= 0.1, (name, order, share)  # (c)


def test_orders_are_what_they_say():
    P = DO.permute
    assert P(DO.cat_first(3, 2), vt="cccuu")["vt"] == "uuccc"
    assert P(DO.alternate(5, 2), vt="cccccuu")["vt"] == "ucucccc" and P(DO.alternate(1, 3), vt="cuuu")["vt"] == "ucuu"
    le = DO.lone_ends(3, 2)
    assert P(le, vt="cccuu")["vt"] == "uccuc" and le[-1] == 0 and le[0] == 4
    for dc, du in ((70, 4), (60, 8)):
        vt = P(DO.straddle(dc, du), vt=DO.cfirst_vt(dc, du))["vt"]
        assert "u" in vt[64:] and "c" in vt[64:] and "u" in vt[:64] and "c" in vt[:64]
    perm = DO.order_perm("random5", 4, 3)
    X = np.arange(14.0).reshape(2, 7)
    out = P(perm, X=X, bw=np.arange(7.0), vt="ccccuuu")
    assert np.array_equal(out["X"][0], perm) and np.array_equal(out["bw"], perm)
    assert out["vt"] == "".join("ccccuuu"[i] for i in perm)


# ---- (a), (c): the grouped cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dc,du,order", DO.group_case_ids())
def test_group_cases_permutation_invariant(dc, du, order):
    c = DO.group_case(dc, du, order)
    assert set(c.kinds.values()) == {"no_model", "const_cont", "one_level", "signed", "unsupported"}
    assert 0 not in c.rows and all(b in c.rows for b in range(1, c.B))
    worst, shares = 0.0, []
    for b in sorted(c.pdf):
        p0s = c.cfirst_pdfs(b)
        diff = np.zeros(p0s[0].shape, dtype=bool)
        for which, p, p0, rows, bw, nlev in zip("lg", c.pdf[b], p0s, c.rows[b], c.bw[b], c.nlev[b]):
            p, p0 = p.reshape(-1), p0.reshape(-1)
            if c.kinds.get(b) == "const_cont":
                assert np.isnan(p).all() and np.isnan(p0).all()
                continue
            data = c.X[c.seg[b]:c.seg[b + 1]][rows]
            bound = DO.pdf_bound(c.D, c.dc, len(data))
            if _signed(bw, c.vt):
                m = 64
                scale = _abs_pdf(data, bw, c.vt, nlev, c.cands[b].reshape(-1, c.D)[:m])
                worst = max(worst, _check_perm(p[:m], p0[:m], bound, (b, which, "signed"), scale=scale))
            else:
                worst = max(worst, _check_perm(p, p0, bound, (b, which)))
                # (d) the log-space restatement, which the grouped ln-pdf is checked against
                m, inv = 12, np.argsort(c.perm)
                data0 = c.X0[c.seg[b]:c.seg[b + 1]][rows]
                lp = O.log_pdf_many(data, bw, c.vt, c.cands[b].reshape(-1, c.D)[:m], nlev)
                lp0 = O.log_pdf_many(data0, bw[inv], c.vt0, c.cands0[b].reshape(-1, c.D)[:m], nlev[inv])
                assert np.array_equal(np.isnan(lp), np.isnan(lp0)) and np.array_equal(np.isfinite(lp), np.isfinite(lp0))
                fin = np.isfinite(lp0)
                lb = _log_bound(data, bw, c.vt, nlev, c.cands[b].reshape(-1, c.D)[:m], lp0)
                assert np.all(np.abs(lp[fin] - lp0[fin]) <= lb[fin]), (b, which, "log_pdf_many")
            diff |= (p.view(np.uint64) != p0.view(np.uint64)).reshape(diff.shape)
        if c.kinds.get(b) != "const_cont":
            pos = np.isfinite(c.pdf[b][0]) & (c.pdf[b][0] > 0)
            shares.append(float((diff & pos).sum()) / max(1, int(pos.sum())))
    print("groups (%d, %d) %s: worst ratio %.3f, order-sensitive shares %s" % (
        dc, du, order, worst, " ".join("%.2f" % s for s in shares)))
    if c.D >= 8:
        assert min(shares) >= 0.1, shares  # (c), in every group that has finite pdfs


# ---- (d): the log-space restatement ----------------------------------------------------------------------------------
def _log_bound(data, bw, vt, nlev, pts, lnp):
    """|ln pdf (permuted) - ln pdf (c-first)| for kde_oracle.log_pdf_many.  Per observation the D log-kernel terms
    are bit-identical and added in dim order: the sums differ by at most (D - 1) 2^-53 T in either order, T the
    largest sum of their magnitudes over the observations.  That absolute error of the exponent is a relative error
    of exp(logk - mx) (plus the subtraction's 2^-53 |logk| <= 2^-53 T and exp's own ulp), kept by the positive
    pairwise sum (ceil(log2 n) + 1 roundings) and the log (one).  The normalisation adds dc logs in dim order
    ((dc + 1) 2^-53 (sum |ln h| + ln n)), and three last additions round at 2^-53 of the largest operand.  Twice
    that, for the two orders."""
    n, D = data.shape
    dc = vt.count("c")
    out = np.empty(len(pts))
    lnh = sum(abs(math.log(bw[d])) for d, t in enumerate(vt) if t == "c") + math.log(n)
    for j, x in enumerate(pts):
        T = np.zeros(n)
        for d, t in enumerate(vt):
            if t == "c":
                T += 0.5 * math.log(2 * math.pi) + (data[:, d] - x[d]) ** 2 / (2 * bw[d] ** 2)
            elif nlev[d] > 1:
                T += np.abs(np.where(data[:, d] == x[d], np.log(abs(1 - bw[d])), np.log(bw[d] / (nlev[d] - 1))))
        T = T.max() * (1 + 1e-9)
        out[j] = 2 * EPS * ((D + 1) * T + 2 + math.ceil(math.log2(n)) + 2 + (dc + 1) * lnh + 3 * (T + lnh + abs(lnp[j])))
    return out


@pytest.mark.parametrize("name,order", [k for k in DO.pair_case_ids() if k[0] != "signed"])
def test_log_pdf_many_permutation_invariant(name, order):
    c = DO.pair_case(name, order)
    m = 48
    worst = 0.0
    for data, bw, nlev, data0, bw0, nlev0, p, p0 in c.kdes():
        lp = O.log_pdf_many(data, bw, c.vt, c.C[:m], nlev)
        lp0 = O.log_pdf_many(data0, bw0, c.vt0, c.C0[:m], nlev0)
        assert np.array_equal(np.isnan(lp), np.isnan(lp0)) and np.array_equal(np.isnan(lp), np.isnan(p[:m]))
        fin = np.isfinite(lp0)
        assert np.array_equal(np.isfinite(lp), fin) and fin.sum() >= 20
        bound = _log_bound(data, bw, c.vt, nlev, c.C[:m], lp0)
        ratio = np.abs(lp[fin] - lp0[fin]) / bound[fin]
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (name, order, ratio.max())
        # ... and it is the ln of the exact pdf where that is representable (a wrong dim in BOTH orders would pass
        # the check above): within the same bound plus the pdf's own and one log
        ok = fin & (p[:m] > TINY)
        tol = bound + DO.pdf_bound(c.D, c.dc, len(data)) + 2 * EPS * (1 + np.abs(lp0))
        assert (np.abs(lp[ok] - np.log(p[:m][ok])) <= tol[ok]).all(), (name, order)
    print("%s %s log_pdf_many: worst ratio to its bound %.3f" % (name, order, worst))


# ---- (d): the cross-validation terms -----------------------------------------------------------------------------
@pytest.mark.parametrize("vt", DO.CV_LAYOUTS)
def test_cv_terms_permutation_invariant(vt):
    """F[i] and L[i] are sums like the pdf's (per-dim factors bit-identical per column -- the convolution kernels
    and the leave-one-out level counts are per column --, D - 1 products, the bandwidth product, one division, a
    pairwise sum of n or n - 1 positive terms): pdf_bound holds as it stands (it allows one division more)."""
    X, pts, X0, vt0, perm = DO.cv_case(vt)
    n, D = X.shape
    bound = DO.pdf_bound(D, vt.count("c"), n)
    rows = list(range(0, n, 3))
    worst = 0.0
    for p in pts:
        p0 = np.empty(D)
        p0[perm] = p
        assert DO.permute(perm, bw=p0)["bw"].tobytes() == p.tobytes()
        F, L = O.cv_terms(X, p, vt, rows=rows)
        F0, L0 = O.cv_terms(X0, p0, vt0, rows=rows)
        for a, b in ((F, F0), (L, L0)):
            a, b = a[rows], b[rows]
            assert np.all(np.isfinite(b)) and np.all(b > 0)
            r = float((np.abs(a - b) / b).max()) / bound
            worst = max(worst, r)
            assert r <= 1.0, (vt, r)
    print("cv_terms %s: worst ratio to the bound %.3f" % (vt, worst))


def test_permutation_check_bites():
    """The check itself: a bandwidth, a level count or a coordinate taken from a neighbouring dim of the same kind
    misses the bound by orders of magnitude."""
    c = DO.pair_case("6c2u", "alternate")
    data, bw, nlev, data0, bw0, nlev0, p, p0 = c.kdes()[0]
    bound = DO.pdf_bound(c.D, c.dc, len(data))
    ci = [i for i, t in enumerate(c.vt) if t == "c"]
    ui = [i for i, t in enumerate(c.vt) if t == "u"]
    ok = p0 > TINY
    for what in ("bw", "nlev", "coord"):
        b2, n2, C2 = bw.copy(), nlev.copy(), c.C.copy()
        if what == "bw":
            b2[ci[0]], b2[ci[1]] = bw[ci[1]], bw[ci[0]]
        elif what == "nlev":
            n2[ui[0]] = nlev[ui[0]] + 1
        else:
            C2[:, [ci[0], ci[1]]] = C2[:, [ci[1], ci[0]]]
        with np.errstate(all="ignore"):
            q = c_oracle.kde_pdf(data, b2, c.vt, n2, C2, exact=True)
        miss = np.abs(q[ok] - p0[ok]) / p0[ok] / bound
        assert np.median(miss) > 1e6, (what, np.median(miss))
