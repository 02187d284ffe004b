"""Continuous and categorical dims interleaved, the single-pair path: fit, every scoring kernel family, the staged
paths, ln-pdf, the host re-score, sharding, cross-validation and the drop-in generator under var_type strings that
are not "c" * dc + "u" * du.

Every case is built c-first by the existing constructors and permuted (tests/dim_orders.py, which
tests/test_oracle_dim_order.py shares: there the oracle is pinned for these very cases and at least one candidate in
ten is shown to have other pdf bits in another column order).  Expected values come from the oracle ON THE PERMUTED
DATA, never from the engine's c-first result: index, score and both pdfs bit for bit.  Every case also builds the
c-first pair and asserts that both pairs' ``variant`` bits are equal, so the kernel family meant is the one that ran.
"""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import kde_oracle as O
from tests import dim_orders as DO
from tests.test_gpu_groups_logpdf import _check_exact, _check_positive
from tests.test_gpu_kde import KERNELS
from tests.test_gpu_rules import _argmin, _bits, _check_pick, _check_topk, _scores, _topk

pytestmark = pytest.mark.gpu

F = 1e-8  # the default score floor


def _orders(name):
    return [(name, o) for o in DO.PAIR_SPECS[name]["orders"]]


def _pairs(case, device):
    """(the pair on the permuted data, the pair on the c-first data)"""
    from hpbandster_amd import kde
    p = kde.fit_pair_from_rows(case.X, case.g_idx, case.b_idx, case.vt, case.bwg, case.bwb, case.nlg, case.nlb,
                               device=device)
    p0 = kde.fit_pair_from_rows(case.X0, case.g_idx, case.b_idx, case.vt0, case.bwg0, case.bwb0, case.nlg0,
                                case.nlb0, device=device)
    return p, p0


def _same_family(p, p0, where):
    """the variant code, the slot counts and the bucket of both pairs"""
    for k, k0 in ((p.good, p0.good), (p.bad, p0.bad)):
        a = (k.variant, k.dc, k.du, k.nconst, k.dc_pad, k.du_pad, k.nan_all)
        b = (k0.variant, k0.dc, k0.du, k0.nconst, k0.dc_pad, k0.du_pad, k0.nan_all)
        assert a == b, (where, a, b)
    print(where, "variant bits good %s bad %s (dc_pad %d du_pad %d kc %d nconst %d)" % (
        bin(p.good.variant), bin(p.bad.variant), p.good.dc_pad, p.good.du_pad, p.good.kc, p.good.nconst))


def _check_surface(pair, case, device, where, seg=64, k=8):
    """acquire, acquire_batch and acquire_topk against the oracle's pdfs of the permuted pool"""
    import torch
    Cd = torch.from_numpy(case.C).to(device)
    nc = len(case.C)
    _check_pick(pair.acquire(Cd), case.l, case.g, F, (where, "acquire"))
    recs = pair.acquire_batch(Cd, seg)
    assert len(recs) == (nc + seg - 1) // seg
    for b, r in enumerate(recs):
        _check_pick(r, case.l[b * seg:(b + 1) * seg], case.g[b * seg:(b + 1) * seg], F, (where, "batch", b))
    _check_topk(pair.acquire_topk(Cd, k), case.l, case.g, F, k, (where, "topk"))


# ---- fit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", _orders("3c1u") + _orders("6c2u") + _orders("24c8u") + _orders("70c4u"))
def test_fit(device, name, order):
    """kde.fit_pair and ObservationStore.refit (rows appended in three steps): the rows are the oracle's split, the
    bandwidths bit-equal to the normal-reference rule on the permuted rows, the level counts np.unique's."""
    from hpbandster_amd import kde
    c = DO.pair_case(name, order)
    g_idx, b_idx = O.bohb_split(c.X, c.losses, c.min_points)
    bwg, bwb = O.normal_reference_bw(c.X[g_idx]), O.normal_reference_bw(c.X[b_idx])
    nlg, nlb = O.num_levels(c.X[g_idx], c.vt), O.num_levels(c.X[b_idx], c.vt)
    store = kde.ObservationStore(c.D, c.vt, device=device)
    n = len(c.X)
    for lo, hi in ((0, n // 2), (n // 2, n // 2 + 1), (n // 2 + 1, n)):
        store.add(c.X[lo:hi], c.losses[lo:hi])
        stepwise = store.refit(c.min_points)
    for pair in (kde.fit_pair(c.X, c.losses, c.vt, c.min_points, device=device), stepwise):
        np.testing.assert_array_equal(pair.good.rows_dev.cpu().numpy(), g_idx)
        np.testing.assert_array_equal(pair.bad.rows_dev.cpu().numpy(), b_idx)
        assert np.array_equal(pair.good.data, c.X[g_idx]) and np.array_equal(pair.bad.data, c.X[b_idx])
        assert np.asarray(pair.good.bw).tobytes() == bwg.tobytes() and np.asarray(pair.bad.bw).tobytes() == bwb.tobytes()
        np.testing.assert_array_equal(pair.good.nlev, nlg)
        np.testing.assert_array_equal(pair.bad.nlev, nlb)
        assert pair.good.dc == c.dc and pair.good.du + pair.good.nconst == c.du


def test_fit_min_bandwidth(device):
    """fit_pair(min_bandwidth=1e-3) on "ccucc": a constant continuous column at dim 0 and a categorical column at dim
    2 that shows one level in the good rows (test_gpu_rules._min_bw_data, permuted): the clipped bandwidths bit for
    bit, and the oracle's picks under them."""
    from hpbandster_amd import kde
    from tests.test_gpu_rules import M, _clip, _min_bw_data, _min_bw_pool, _pair_oracle
    perm = np.array([1, 0, 4, 2, 3])
    vt = DO.permute(perm, vt="ccccu")["vt"]
    assert vt == "ccucc"
    n = 120
    rs = np.random.RandomState(5)
    losses = rs.rand(n)
    good = np.argsort(losses)[:(15 * n) // 100]
    X = DO.permute(perm, X=_min_bw_data(rs, n, good))["X"]
    pm = kde.fit_pair(X, losses, vt, 6, device=device, min_bandwidth=M)
    g_idx, b_idx = O.bohb_split(X, losses, 6)
    assert np.array_equal(pm.good.data, X[g_idx]) and np.array_equal(pm.bad.data, X[b_idx])
    with np.errstate(all="ignore"):
        rawg, rawb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    assert rawg[0] == 0.0 and rawg[2] == 0.0 and 0 < rawg[3] < M and rawg[1] > M and rawg[4] > M
    bwg, bwb = _clip(rawg, M), _clip(rawb, M)
    assert np.asarray(pm.good.bw).tobytes() == bwg.tobytes() and np.asarray(pm.bad.bw).tobytes() == bwb.tobytes()
    np.testing.assert_array_equal(pm.good.nlev, O.num_levels(X[g_idx], vt))
    np.testing.assert_array_equal(pm.bad.nlev, O.num_levels(X[b_idx], vt))
    assert pm.good.nlev[2] == 1 and pm.bad.nlev[2] == 4 and pm.good.exact_only and not pm.bad.exact_only
    inv = np.argsort(perm)
    C0, mis = _min_bw_pool(np.random.RandomState(6), X[g_idx][:, inv], 64)
    C = DO.permute(perm, C=C0)["C"]
    l, g = _pair_oracle(pm, vt, C, bwg, bwb)
    assert np.isinf(l[mis]).all() and mis.sum() >= 3 and np.isfinite(l[~mis]).all()
    _check_pick(pm.acquire(C), l, g, F, "min_bandwidth acquire")
    for b, r in enumerate(pm.acquire_batch(C, 16)):
        _check_pick(r, l[16 * b:16 * b + 16], g[16 * b:16 * b + 16], F, ("min_bandwidth batch", b))
    _check_topk(pm.acquire_topk(C, 8), l, g, F, 8, "min_bandwidth topk")
    keep = ~mis
    _check_pick(pm.acquire(np.ascontiguousarray(C[keep])), l[keep], g[keep], F, "min_bandwidth matching pool")


# ---- acquisition, per kernel family ------------------------------------------------------------------------------
# (case, kernel switches of test_gpu_kde.KERNELS or None for the default selection)
FAMILIES = [("3c1u", None), ("6c2u", None), ("24c8u", None), ("signed", None),
            ("16c8u3", "h32"), ("16c8u3", "h16"), ("16c8u3", "f32"), ("24c8u", "h32"), ("24c8u", "h16"),
            ("24c8u", "f32"), ("oh20", "h32"), ("oh20", "h16"), ("oh24", "h32"), ("oh24", "h16"),
            ("f32oh12", "f32"), ("f32valu33", "f32"), ("70c4u", None), ("3c33u", None), ("const8", None),
            ("const24", None)]


@pytest.mark.parametrize("name,kernel,order", [(n, k, o) for n, k in FAMILIES for o in DO.PAIR_SPECS[n]["orders"]])
def test_acquire_families(device, monkeypatch, name, kernel, order):
    if kernel is not None:
        for key, v in KERNELS[kernel].items():
            monkeypatch.setenv(key, v)
    c = DO.pair_case(name, order)
    pair, pair0 = _pairs(c, device)
    _same_family(pair, pair0, (name, kernel, order, c.vt))
    for kd in (pair.good, pair.bad):
        f16, t32, coarse = (kd.variant >> 4) & 1, (kd.variant >> 6) & 1, (kd.variant >> 7) & 1
        if name == "3c1u" or kernel == "f32":
            assert not f16  # the f32 kernels
        if name == "6c2u" or kernel in ("h32", "h16"):
            assert f16  # the f16 matrix-core kernels
        if kernel == "h16":
            assert not t32
        if name == "24c8u" and kernel is None:
            assert coarse  # the coarse 32x32 instance
        if name == "signed":
            assert kd.has_neg
        if name in ("70c4u", "3c33u"):
            assert kd.exact_only
        if name in ("const8", "const24"):
            assert kd.nconst == 1 and kd.du == 2 and not kd.exact_only
        if name == "f32oh12":
            assert kd.kc == 4
        if name == "f32valu33":
            assert kd.kc == 0 and kd.dc_pad == 64
    if name.startswith("const"):
        assert np.isnan(c.l).any() and np.isfinite(c.l).sum() > 400  # off the one level: 0 / 0
    _check_surface(pair, c, device, (name, kernel, order))


# ---- staged ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", _orders("staged"))
def test_staged(device, monkeypatch, name, order):
    """HBX_STAGED=2 against 0 at 4099 candidates: the argmin's and the top-k's records are equal, and the oracle's."""
    import torch
    c = DO.pair_case(name, order)
    pair, pair0 = _pairs(c, device)
    _same_family(pair, pair0, (name, order))
    Cd, nc, k = torch.from_numpy(c.C).to(device), len(c.C), 8
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)
    wk = torch.empty(pair.topk_workspace_bytes(nc, k), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "0")
    off = pair.acquire(Cd, workspace=ws)
    assert not pair.acquire_stats(ws, nc)["staged"]
    toff = pair.acquire_topk(Cd, k, workspace=wk)
    monkeypatch.setenv("HBX_STAGED", "2")
    on = pair.acquire(Cd, workspace=ws)
    st = pair.acquire_stats(ws, nc)
    assert st["staged"], st
    ton = pair.acquire_topk(Cd, k, workspace=wk)
    assert pair.acquire_stats(wk, nc)["staged"]
    for r in (on, off):
        _check_pick(r, c.l, c.g, F, (order, "staged argmin"))
    assert (on.index, _bits(on.score), _bits(on.pdf_l), _bits(on.pdf_g), on.flags, on.near) == \
        (off.index, _bits(off.score), _bits(off.pdf_l), _bits(off.pdf_g), off.flags, off.near)
    for t in (ton, toff):
        _check_topk(t, c.l, c.g, F, k, (order, "staged topk"))
    assert (ton.count, ton.flags) == (toff.count, toff.flags)
    for fld in ("index", "score", "pdf_l", "pdf_g", "rel"):
        assert getattr(ton, fld)[:ton.count].tobytes() == getattr(toff, fld)[:toff.count].tobytes(), fld


@pytest.mark.parametrize("name,order", _orders("split"))
def test_observation_splits(device, monkeypatch, name, order):
    """64 candidates against 10000 observations: the blocks split the observations into ranges (HBX_OBS_SPLIT=1);
    the record is the unsplit launch's and the oracle's, single and batched."""
    import torch
    c = DO.pair_case(name, order)
    pair, pair0 = _pairs(c, device)
    _same_family(pair, pair0, (name, order))
    Cd = torch.from_numpy(c.C).to(device)

    def rec(r):
        return (r.index, _bits(r.score), _bits(r.pdf_l), _bits(r.pdf_g))
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")
    one = pair.acquire(Cd)
    rb0 = pair.acquire_batch(Cd, 16)
    monkeypatch.setenv("HBX_OBS_SPLIT", "1")
    two = pair.acquire(Cd)
    rb1 = pair.acquire_batch(Cd, 16)
    assert rec(one) == rec(two) and [rec(a) for a in rb0] == [rec(b) for b in rb1]
    _check_pick(two, c.l, c.g, F, (order, "split"))
    for b, r in enumerate(rb1):
        _check_pick(r, c.l[16 * b:16 * b + 16], c.g[16 * b:16 * b + 16], F, (order, "split batch", b))


# ---- ln-pdf ----------------------------------------------------------------------------------------------------------
_LOG_REFS = {}


def _log_refs(c, m):
    """per KDE: (data, bw, nlev, the log-space oracle, the exact pdf) of the first m candidates, computed once"""
    key = (id(c), m)
    if key not in _LOG_REFS:
        out = []
        for data, bw, nlev, _, _, _, p, _ in c.kdes():
            out.append((O.log_pdf_many(data, bw, c.vt, c.C[:m], nlev), p[:m]))
        _LOG_REFS[key] = out
    return _LOG_REFS[key]


@pytest.mark.parametrize("lut", ["1", "0"])
@pytest.mark.parametrize("name,order", _orders("24c8u") + _orders("8c8u4") + _orders("signed"))
def test_logpdf(device, monkeypatch, name, order, lut):
    """DeviceKDE.logpdf (hbx_kde_logpdf_rtol) at rtol 1e-5 and 1e-9, with the direct-difference pass's code tables
    on and off: against the log-space oracle, and against ln of the exact pdf where that is a normal number."""
    monkeypatch.setenv("HBX_DD_LUT", lut)
    c = DO.pair_case(name, order)
    pair, pair0 = _pairs(c, device)
    _same_family(pair, pair0, (name, order, "lut", lut))
    m = 160
    C = np.ascontiguousarray(c.C[:m])
    for kd, (lsp, ex) in zip((pair.good, pair.bad), _log_refs(c, m)):
        for rtol in (1e-5, 1e-9):
            got = kd.logpdf(C, rtol=rtol)
            tag = (name, order, lut, rtol)
            if name == "signed":
                assert kd.has_neg
                with np.errstate(all="ignore"):
                    _check_exact(got, np.log(ex), ex, lsp, tag)
                continue
            _check_positive(got, lsp, rtol, tag)
            ok = ex > 1e-300
            err = np.abs(got[ok] - np.log(ex[ok])) / np.maximum(1.0, np.abs(np.log(ex[ok])))
            assert ok.sum() > 40 and err.max() <= rtol, (tag, err.max())


# ---- host re-score and sharding --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", _orders("6c2u") + _orders("24c8u"))
def test_host_rescore_and_sharding(device, name, order):
    """exact_host.kde_pdf (this numpy's expressions in the reference's dim order) for the winner: bit-equal to the
    numpy transcription of the oracle on the permuted data, and within 4 ulp per continuous dim of the record's pdfs
    (this numpy's exp is not the pinned 1.26.4 one, 1 ulp apart at most; everything else is the same operation in the
    same order).  exact_host.resolve over the eight best picks the oracle's winner.  A 3-way sharded pick
    (index_base) reduces to the whole-pool pick."""
    from hpbandster_amd import exact_host as E
    c = DO.pair_case(name, order)
    pair, _ = _pairs(c, device)
    res = pair.acquire(c.C)
    want = _check_pick(res, c.l, c.g, F, (name, order))
    tol = 4 * c.dc * 2.0 ** -52
    for kd, rec in ((pair.good, res.pdf_l), (pair.bad, res.pdf_g)):
        h = float(E.kde_pdf(kd.data, kd.bw, kd.var_type, kd.nlev, c.C[want]))
        assert _bits(h) == _bits(O.pdf(kd.data, kd.bw, c.vt, c.C[want], kd.nlev))
        assert abs(h - rec) <= tol * rec, (name, order, h, rec)
    idx = _topk(_scores(c.l, c.g, F), 8)
    pick = E.resolve(pair.good, pair.bad, c.C[idx], idx)
    s = _scores(c.l, c.g, F)
    assert pick[0] == want or abs(s[pick[0]] - s[want]) <= 2 * tol * s[want], (pick, want)
    nc = len(c.C)
    cuts = [0, nc // 3, (2 * nc) // 3, nc]
    best = (np.inf, -1)
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = pair.acquire(np.ascontiguousarray(c.C[a:b]), index_base=a)
        if r.index >= 0 and (r.score < best[0] or (r.score == best[0] and r.index < best[1])):
            best = (r.score, r.index)
    assert best[1] == want and _bits(best[0]) == _bits(res.score)


# ---- cross-validation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt", DO.CV_LAYOUTS)
def test_cv_terms(device, vt):
    from hpbandster_amd.cv import CVObjective
    X, pts, _, _, _ = DO.cv_case(vt)
    obj = CVObjective(X, vt, device=device)
    np.testing.assert_array_equal(obj.normal_reference(), O.normal_reference_bw(X))
    for p in pts:
        Fg, Lg = obj.terms(p)
        Fo, Lo = O.cv_terms(X, p, vt)
        np.testing.assert_allclose(Fg, Fo, rtol=1e-13, atol=0)
        np.testing.assert_allclose(Lg, Lo, rtol=1e-13, atol=0)


@pytest.mark.parametrize("vt,n", [(DO.CV_LAYOUTS[0], 40), (DO.CV_LAYOUTS[1], 40), (DO.CV_LAYOUTS[2], 16)])
def test_cv_ml_bandwidth(device, vt, n):
    """select_bandwidth('cv_ml') against the oracle's Nelder-Mead over its own objective (16 rows at 12 dims: the
    host's thousand objective evaluations take seconds)."""
    from hpbandster_amd.cv import select_bandwidth
    X = DO.cv_case(vt, n=n)[0]
    bw = select_bandwidth(X, vt, "cv_ml", device=device)
    np.testing.assert_allclose(bw, O.cv_bandwidth(X, vt, "cv_ml"), rtol=1e-6)


# ---- the drop-in generator -----------------------------------------------------------------------------------------
class _Job(object):
    pass


@pytest.mark.parametrize("sampler", ["host", "gpu"])
def test_bohb_drop_in_interleaved_names(device, sampler):
    """BOHB on a space whose sorted names interleave the kinds (a_cat, b_x, c_cat, d_x, e_x, f_cat -> "ucuccu"): the
    configuration returned is the oracle's selection over the candidates the call drew."""
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB
    from hpbandster_amd.configspace import Configuration
    space = CS.ConfigurationSpace(seed=3)
    for nm in ("e_x", "b_x", "d_x"):
        space.add_hyperparameter(CS.UniformFloatHyperparameter(nm, lower=-2, upper=3))
    for nm, ch in (("f_cat", ["p", "q", "r"]), ("a_cat", ["a", "b", "c", "d"]), ("c_cat", ["s", "t"])):
        space.add_hyperparameter(CS.CategoricalHyperparameter(nm, ch))
    cg = BOHB(space, device=device, random_fraction=0.0, num_samples=64, sampler=sampler, sampler_seed=17)
    assert list(space.get_hyperparameter_names()) == ["a_cat", "b_x", "c_cat", "d_x", "e_x", "f_cat"]
    assert cg.kde_vartypes == "ucuccu" and list(cg.vartypes) == [4, 0, 2, 0, 0, 3]
    rs = np.random.RandomState(3)
    for k in range(80):
        cfg = space.sample_configuration().get_dictionary()
        j = _Job()
        j.id, j.exception, j.timestamps = (0, 0, k), None, {}
        j.kwargs = {"config": cfg, "budget": 1.0}
        j.result = {"loss": float(rs.rand()) + (cfg["b_x"] - 1.0) ** 2 + (0.0 if cfg["a_cat"] == "a" else 1.0),
                    "info": None}
        cg.new_result(j)
    pair = cg.kde_models[1.0]
    vt = cg.kde_vartypes
    bwg, bwb = O.normal_reference_bw(pair.good.data), O.normal_reference_bw(pair.bad.data)
    assert np.asarray(pair.good.bw).tobytes() == bwg.tobytes() and np.asarray(pair.bad.bw).tobytes() == bwb.tobytes()
    np.testing.assert_array_equal(pair.good.nlev, O.num_levels(pair.good.data, vt))
    np.testing.assert_array_equal(pair.bad.nlev, O.num_levels(pair.bad.data, vt))
    np.random.seed(7)
    counter = cg._sample_counter
    cfg, info = cg.get_config(1.0)
    assert info["model_based_pick"]
    if sampler == "host":
        np.random.seed(7)
        np.random.rand()
        cands = np.array(cg.sample_candidates(pair["good"], cg.num_samples))
    else:
        cands = pair.good.sample(cg.vartypes, cg.bw_factor, cg.num_samples, cg.sampler_seed, counter)[0].cpu().numpy()
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(pair.good.data, bwg, vt, pair.good.nlev, cands, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, bwb, vt, pair.bad.nlev, cands, exact=True)
    want = _argmin(_scores(l, g, F))
    assert want >= 0
    assert cfg == Configuration(space, vector=cands[want]).get_dictionary()
    # the draws keep every dim in its own kind: categorical codes in range, continuous dims truncated normals (the
    # reference's bounds are in units of h and its scale 3 h, so they may leave [0, 1])
    for d, lv in enumerate(cg.vartypes):
        col = cands[:, d]
        if lv:
            assert np.all((col == np.floor(col)) & (col >= 0) & (col < lv)), d
        else:
            assert np.unique(col).size > 32 and np.any(col != np.floor(col)), d
