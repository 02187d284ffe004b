"""Grouped ln-pdf (hbx_kde_logpdf_groups, GroupModel.logpdf) on the GPU: both KDEs' log densities of every group's
pool, against the fp64 log-space oracle (kde_oracle.log_pdf_many) for KDEs with positive factors and against ln of
the reference's own fp64 pdf (c_oracle.kde_pdf(exact=True)) for the EXACT ones, in default and FP64_ONLY mode.
"""
import functools

import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import SHAPES, _groups

pytestmark = pytest.mark.gpu

NO_MODEL, UNSUPPORTED, EXACT_L, EXACT_G = 16, 32, 64, 128
POOLS = [1, 70]  # 70 straddles a 64-candidate tile


@functools.lru_cache(maxsize=None)
def _case(device, dc, du, C):
    """The ragged groups of test_gpu_groups, fitted once, with the per-(group, KDE) references computed once:
    refs[(b, kd)] = (exact, ref, ex, lsp) -- `exact`: the KDE is one the engine takes through the exact pdf; `ref`:
    what the values are checked against; `ex`: the reference's fp64 pdf (exact KDEs); `lsp`: the log-space oracle."""
    from oracle import c_oracle
    from hpbandster_amd import groups
    X, losses, seg, vt, levels, cands, kinds = _groups(dc, du, C)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    bws = gm.bandwidths()
    nls = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    cat = np.array([v == "u" for v in vt])
    refs = {}
    for b in range(gm.B):
        if kinds.get(b) in ("no_model", "unsupported"):
            continue
        Xb = X[seg[b]:seg[b + 1]]
        for kd, rows in enumerate(gm.rows_of(b)):
            bw, nl = bws[kd][b], nls[kd][b]
            data = Xb[rows]
            # KDEs the engine takes through ln of its exact fp64 pdf (test_gpu_fuzz.py::test_random_logpdf_contract's
            # rule): a negative match factor, or a categorical dim with a single observed level
            exact = bool(np.any((bw[cat] > 1.0) & (nl[cat] > 1)) or np.any(nl[cat] == 1))
            lsp = O.log_pdf_many(data, bw, vt, cands[b], nl)
            ex = None
            ref = lsp
            if exact:
                with np.errstate(all="ignore"):
                    ex = c_oracle.kde_pdf(data, bw, vt, nl, cands[b], exact=True)
                    ref = np.log(ex)
            refs[(b, kd)] = (exact, ref, ex, lsp)
    return dict(gm=gm, cands=cands, kinds=kinds, refs=refs, B=gm.B, C=C)


@functools.lru_cache(maxsize=None)
def _run(device, dc, du, C, fp64_only):
    return _case(device, dc, du, C)["gm"].logpdf(_case(device, dc, du, C)["cands"], fp64_only=fp64_only)


def _within(got, ref, rtol):
    with np.errstate(invalid="ignore"):
        return np.abs(got - ref) <= rtol * np.maximum(1.0, np.abs(ref))


def _check_positive(got, ref, rtol, tag):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=str(tag))
    ninf = np.isneginf(ref)
    assert np.all(np.isneginf(got[ninf])), tag
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(got[fin])), tag
    err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    print("%s: max error %.3g of %.3g" % (tag, err.max(initial=0.0), rtol))
    assert err.max(initial=0.0) <= rtol, (tag, err.max())


def _check_exact(got, ref, ex, lsp, tag):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=str(tag))
    with np.errstate(invalid="ignore"):
        normal = ex > 1e-300
        zero = ex == 0
        tiny = (ex > 0) & ~normal
    assert np.all(_within(got[normal], ref[normal], 1e-12)), (tag, got[normal], ref[normal])
    assert np.all(_within(got[tiny], ref[tiny], 1e-5)), tag  # (a subnormal pdf: the contract's own tolerance)
    gz = got[zero]
    assert np.all(np.isneginf(gz) | (np.isfinite(gz) & np.isfinite(lsp[zero]) & _within(gz, lsp[zero], 1e-5))), \
        (tag, gz, lsp[zero])


@pytest.mark.parametrize("fp64_only", [False, True])
@pytest.mark.parametrize("C", POOLS)
@pytest.mark.parametrize("dc,du", SHAPES)
def test_contract_against_the_oracles(device, dc, du, C, fp64_only):
    case = _case(device, dc, du, C)
    r = _run(device, dc, du, C, fp64_only)
    B, kinds = case["B"], case["kinds"]
    assert r.ln_l.shape == (B, C) and r.ln_g.shape == (B, C) and r.status.shape == (B,)
    assert r.ln_l.dtype == np.float64 and r.status.dtype == np.int32
    for b in range(B):
        kind = kinds.get(b)
        if kind in ("no_model", "unsupported"):
            assert r.status[b] & (NO_MODEL if kind == "no_model" else UNSUPPORTED), (b, kind, r.status[b])
            assert np.all(np.isnan(r.ln_l[b])) and np.all(np.isnan(r.ln_g[b])), (b, kind)
            continue
        assert not r.status[b] & (NO_MODEL | UNSUPPORTED), (b, kind, r.status[b])
        for kd, got in enumerate((r.ln_l[b], r.ln_g[b])):
            exact, ref, ex, lsp = case["refs"][(b, kd)]
            tag = (dc, du, C, fp64_only, b, kind, "g" if kd else "l")
            if exact:
                assert r.status[b] & (EXACT_G if kd else EXACT_L), tag
                _check_exact(got, ref, ex, lsp, tag)
            else:
                _check_positive(got, ref, 1e-5, tag)
            if kind == "const_cont":
                assert np.all(np.isnan(got)) and np.all(np.isnan(ref)), tag
        if kind == "signed":
            assert r.status[b] & EXACT_L, (b, r.status[b])
        if kind == "one_level":
            assert r.status[b] & (EXACT_L | EXACT_G), (b, r.status[b])
        if du == 0 and kind != "const_cont":
            assert r.status[b] == 0, (b, r.status[b])  # continuous dims with positive bandwidths: no exact path


@pytest.mark.parametrize("C", POOLS)
@pytest.mark.parametrize("dc,du", SHAPES)
def test_default_mode_against_fp64_only(device, dc, du, C):
    case = _case(device, dc, du, C)
    a, f = _run(device, dc, du, C, False), _run(device, dc, du, C, True)
    B = case["B"]
    np.testing.assert_array_equal(a.status, f.status)
    for x, y in ((a.ln_l, f.ln_l), (a.ln_g, f.ln_g)):
        np.testing.assert_array_equal(np.isnan(x), np.isnan(y))
        np.testing.assert_array_equal(np.isneginf(x), np.isneginf(y))
        fin = np.isfinite(y)
        assert np.all(np.isfinite(x[fin]))
        assert np.all(np.abs(x[fin] - y[fin]) <= 2e-5 * np.maximum(1.0, np.abs(y[fin])))
    print("stats (%d, %d) C = %d: default %s, fp64 only %s" % (dc, du, C, a.stats, f.stats))
    assert sum(a.stats) == 2 * B * C and sum(f.stats) == 2 * B * C
    assert f.stats[0] == 0
    assert a.stats[3] == f.stats[3] and a.stats[2] == f.stats[2]
    if (dc, du) == (8, 0):
        assert a.stats[0] > 0  # the fp32 pass certifies something (the share is recorded in DESIGN, not asserted)


@pytest.mark.parametrize("dc,du", [(5, 2), (8, 0)])  # (5, 2): most categorical KDEs there are signed; (8, 0): none
def test_tighter_rtol(device, dc, du):
    C = 70
    case = _case(device, dc, du, C)
    r = case["gm"].logpdf(case["cands"], rtol=1e-9, fp64_only=False)
    checked = 0
    for (b, kd), (exact, ref, ex, lsp) in case["refs"].items():
        if exact:
            continue
        _check_positive((r.ln_g if kd else r.ln_l)[b], ref, 1e-9, ("rtol 1e-9", b, kd))
        checked += 1
    assert checked >= (2 if du else 40)


@pytest.mark.parametrize("dc,du,lev", [(24, 8, 2), (40, 6, 3)])
def test_unsigned_categorical_buckets(device, dc, du, lev):
    """The ragged builder's categorical KDEs at D = 32 are all signed (exact path).  Few levels keep every
    bandwidth below 1, so the 32-slot instances (24c + 8u: config #5's piece counts) and the 64 + 32-slot ones
    (D = 46) run both passes with categorical dims, against the log-space oracle."""
    from hpbandster_amd import groups
    from hpbandster_amd import synthetic as S
    lens = np.array([dc + du + 2, 200, 330])  # chunk ends: one partial chunk, 3 chunks + 8, 5 chunks + 10
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    C, D = 70, dc + du
    X = S.make_observations(int(seg[-1]), dc, du, lev, seed=31)
    losses = S.make_losses(int(seg[-1]), seed=32)
    vt = S.var_type_string(dc, du)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    rs = np.random.RandomState(33)
    cands = S.make_candidates(len(lens) * C, dc, du, lev, seed=34).reshape(len(lens), C, D)
    for b in range(len(lens)):  # near an observation, and observation rows themselves
        src = X[seg[b]:seg[b + 1]][rs.randint(0, lens[b], size=C // 2)]
        cands[b, :C // 2] = src
        cands[b, :C // 4, :dc] += 0.01 * rs.randn(C // 4, dc)
    bws = gm.bandwidths()
    nls = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    runs = [gm.logpdf(cands, fp64_only=False), gm.logpdf(cands, fp64_only=True)]
    print("stats (%d, %d): default %s, fp64 only %s" % (dc, du, runs[0].stats, runs[1].stats))
    for r in runs:
        assert np.all(r.status == 0), r.status
        assert sum(r.stats) == 2 * len(lens) * C and r.stats[2] == 0 and r.stats[3] == 0
        for b in range(len(lens)):
            Xb = X[seg[b]:seg[b + 1]]
            for kd, rows in enumerate(gm.rows_of(b)):
                ref = O.log_pdf_many(Xb[rows], bws[kd][b], vt, cands[b], nls[kd][b])
                _check_positive((r.ln_g if kd else r.ln_l)[b], ref, 1e-5, (dc, du, b, kd))
    assert runs[1].stats[0] == 0


def test_plumbing(device):
    import torch
    from hpbandster_amd import groups
    dc, du, C = 5, 2, 70
    case = _case(device, dc, du, C)
    gm, cands, B, D = case["gm"], case["cands"], case["B"], dc + du
    both = _run(device, dc, du, C, False)
    # which: the other output is None, the requested one is the "both" call's bit for bit
    good = gm.logpdf(cands, which="good", fp64_only=False)
    bad = gm.logpdf(cands, which="bad", fp64_only=False)
    assert good.ln_g is None and bad.ln_l is None
    assert good.ln_l.tobytes() == both.ln_l.tobytes() and bad.ln_g.tobytes() == both.ln_g.tobytes()
    assert sum(good.stats) == B * C and sum(bad.stats) == B * C
    # two identical calls are bit-identical
    again = gm.logpdf(cands, fp64_only=False)
    assert again.ln_l.tobytes() == both.ln_l.tobytes() and again.ln_g.tobytes() == both.ln_g.tobytes()
    np.testing.assert_array_equal(again.status, both.status)
    # [B, S, C, D] equals the flattened [B, S * C, D] call bit for bit
    S = 2
    four = gm.logpdf(cands.reshape(B, S, C // S, D), fp64_only=False)
    assert four.ln_l.shape == (B, S, C // S) and four.ln_g.shape == (B, S, C // S)
    assert four.ln_l.tobytes() == both.ln_l.tobytes() and four.ln_g.tobytes() == both.ln_g.tobytes()
    # a device-tensor pool, sync=False, a non-default stream: the same bytes
    st = torch.cuda.Stream(device=device)
    cd = torch.from_numpy(np.ascontiguousarray(cands)).to(device)
    torch.cuda.synchronize(device)
    dev = gm.logpdf(cd, stream=st, sync=False, fp64_only=False)
    assert dev.stats is None and dev.ln_l.is_cuda and dev.status.is_cuda
    st.synchronize()
    assert dev.ln_l.cpu().numpy().tobytes() == both.ln_l.tobytes()
    assert dev.ln_g.cpu().numpy().tobytes() == both.ln_g.tobytes()
    np.testing.assert_array_equal(dev.status.cpu().numpy(), both.status)
    with pytest.raises(Exception):
        gm.logpdf(cd.to(torch.float32))
    with pytest.raises(Exception):
        gm.logpdf(cands[:, :, :D - 1])
    # the Python default is the fp64 pass alone (the fp32 pass does not pay at every shape)
    dflt = gm.logpdf(cands)
    assert dflt.stats[0] == 0 and sum(dflt.stats) == 2 * B * C
    assert dflt.ln_l.tobytes() == _run(device, dc, du, C, True).ln_l.tobytes()
    # C == 0 and B == 0: empty arrays
    e = gm.logpdf(np.empty((B, 0, D)))
    assert e.ln_l.shape == (B, 0) and e.ln_g.shape == (B, 0) and e.status.shape == (B,) and e.stats == (0, 0, 0, 0)
    g0 = groups.fit_groups(np.empty((0, D)), np.empty(0), np.zeros(1, np.int64), "c" * dc + "u" * du, device=device)
    e0 = g0.logpdf(np.empty((0, 5, D)))
    assert e0.ln_l.shape == (0, 5) and e0.ln_g.shape == (0, 5) and len(e0) == 0


def test_agreement_with_the_single_path(device):
    dc, du, C = 24, 8, 70
    case = _case(device, dc, du, C)
    gm, cands, kinds = case["gm"], case["cands"], case["kinds"]
    r = _run(device, dc, du, C, False)
    plain = [b for b in range(case["B"]) if kinds.get(b) is None]
    plain = ([b for b in plain if r.status[b] == 0] or plain)[0]  # (no exact path, where such a group exists)
    signed = next(b for b, k in kinds.items() if k == "signed")
    long_ = next(b for b, k in kinds.items() if k == "long")
    for b in (plain, signed, long_):
        pair = gm.pair(b)
        for got, k in ((r.ln_l[b], pair.good), (r.ln_g[b], pair.bad)):
            one = k.logpdf(cands[b])
            np.testing.assert_array_equal(np.isnan(got), np.isnan(one))
            fin = np.isfinite(one) & np.isfinite(got)
            # (-inf on one side and a finite log-space value on the other: both are accepted where the fp64 pdf
            # underflows to 0; everything else must be finite on both sides)
            odd = ~np.isnan(one) & ~fin
            assert np.all(np.isneginf(one[odd]) | np.isneginf(got[odd])), (b, one[odd], got[odd])
            assert np.all(np.abs(got[fin] - one[fin]) <= 2e-5 * np.maximum(1.0, np.abs(one[fin]))), b
