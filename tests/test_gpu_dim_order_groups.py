"""Continuous and categorical dims interleaved, the grouped path: fit_groups, the grouped records (acquire,
acquire_requests under both screens, acquire_topk, gm.pair(b).acquire), logpdf, sampling, get_config and GroupBOHB.

B = 6 ragged groups of test_gpu_groups._groups' recipe (no model, a constant continuous column, one observed level,
signed, unsupported codes, a plain group), permuted after construction (tests/dim_orders.GroupCase, shared with
tests/test_oracle_dim_order.py, which pins the oracle for these cases); C = 65, S = 3, k = 5; one shape per slot
bucket and pair loop, past 64 dims with both kinds on both sides of dim 64.  Expected values: the oracle on the
permuted data -- the split, the bandwidths and the level counts included, so the models the records are checked
under are not the engine's own.
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests import dim_orders as DO
from tests.test_gpu_groups_logpdf import _check_exact, _check_positive
from tests.test_gpu_rules import _argmin, _bits, _scores, _topk

pytestmark = pytest.mark.gpu

NO_MODEL, UNSUPPORTED, EXACT_L, EXACT_G = 16, 32, 64, 128
SRC_MODEL = 0
F = 1e-8
CASES = DO.group_case_ids()
_GM = {}


def _fit(c, device):
    from hpbandster_amd import groups
    key = (c.dc, c.du, c.order)
    if key not in _GM:
        _GM[key] = groups.fit_groups(c.X, c.losses, c.seg, c.vt, device=device)
    return _GM[key]


def _want_nlev(data, vt):
    """np.unique's count per categorical column, -1 where a code is not an integer (the engine's mark)"""
    return np.array([0 if t == "c" else (-1 if (data[:, d] != np.floor(data[:, d])).any() else
                                         np.unique(data[:, d]).size) for d, t in enumerate(vt)])


def _check_fit(gm, c):
    bws = gm.bandwidths()
    nls = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    for b in range(c.B):
        assert bool(gm.has_model[b]) == (b in c.rows), b
        if b not in c.rows:
            assert gm.n_good[b] == 0 and gm.n_bad[b] == 0
            continue
        Xb = c.X[c.seg[b]:c.seg[b + 1]]
        for kd, rows in enumerate(gm.rows_of(b)):
            np.testing.assert_array_equal(rows, c.rows[b][kd])
            assert bws[kd][b].tobytes() == c.bw[b][kd].tobytes(), (b, kd, bws[kd][b], c.bw[b][kd])
            np.testing.assert_array_equal(nls[kd][b], _want_nlev(Xb[c.rows[b][kd]], c.vt))
            if c.kinds.get(b) != "unsupported":
                np.testing.assert_array_equal(nls[kd][b], c.nlev[b][kd])


@pytest.mark.parametrize("dc,du,order", CASES)
def test_fit_groups(device, dc, du, order):
    c = DO.group_case(dc, du, order)
    gm = _fit(c, device)
    assert gm.B == c.B and gm.D == c.D
    _check_fit(gm, c)
    cat = np.array([t == "u" for t in c.vt])
    assert np.any(c.bw[3][0][cat] > 1.0)  # the signed group is signed


def test_fit_groups_wave_kernel_mixed_vartype(device):
    """B = 1700 groups of D = 5, "ucucc": 2 B D = 17000 >= 16384 columns, the wave-per-column fit kernel."""
    from hpbandster_amd import groups
    B, n, vt = 1700, 40, "ucucc"
    rs = np.random.RandomState(1700)
    X = rs.rand(B * n, 5)
    for d, t in enumerate(vt):
        if t == "u":
            X[:, d] = rs.randint(0, 3 + d, size=B * n)
    losses = rs.rand(B * n)
    seg = np.arange(B + 1, dtype=np.int64) * n
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    bws = gm.bandwidths()
    nls = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    for b in range(B):
        sp = DO.group_split(losses[seg[b]:seg[b + 1]], 5)
        Xb = X[seg[b]:seg[b + 1]]
        if b % 100 == 0:
            for kd, rows in enumerate(gm.rows_of(b)):
                np.testing.assert_array_equal(rows, sp[kd])
        for kd in (0, 1):
            assert bws[kd][b].tobytes() == O.normal_reference_bw(Xb[sp[kd]]).tobytes(), (b, kd)
            np.testing.assert_array_equal(nls[kd][b], O.num_levels(Xb[sp[kd]], vt))


def _check_records(c, gm, monkeypatch, with_pairs=True):
    B, S, C, k = c.B, DO.GROUP_S, DO.GROUP_C, DO.GROUP_K
    one = gm.acquire(np.ascontiguousarray(c.cands[:, 0]))
    reqs = {}
    for screen in ("1", "2"):
        monkeypatch.setenv("HBX_GROUPS_SCREEN", screen)
        reqs[screen] = gm.acquire_requests(c.cands)
    monkeypatch.delenv("HBX_GROUPS_SCREEN")
    top = gm.acquire_topk(np.ascontiguousarray(c.cands[:, 1]), k)
    scored = 0
    for b in range(B):
        kind = c.kinds.get(b)
        if kind in ("no_model", "unsupported"):
            flag = NO_MODEL if kind == "no_model" else UNSUPPORTED
            assert one.index[b] == -1 and one.flags[b] & flag, (b, kind)
            for req in reqs.values():
                assert np.all(req.index[b] == -1) and np.all(req.flags[b] & flag), (b, kind)
            assert top.count[b] == 0
            continue
        l, g = c.pdf[b]
        pair = gm.pair(b) if with_pairs else None
        for s in range(S):
            sc = _scores(l[s], g[s], F)
            want = _argmin(sc)
            recs = [(req, (b, s), "requests screen " + key) for key, req in reqs.items()]
            if s == 0:
                recs.append((one, b, "acquire"))
            for rec, at, what in recs:
                assert rec.index[at] == want, (b, kind, s, what, rec.index[at], want)
                if want < 0:
                    continue
                assert _bits(rec.score[at]) == _bits(sc[want]), (b, kind, s, what)
                assert _bits(rec.pdf_l[at]) == _bits(l[s][want]) and _bits(rec.pdf_g[at]) == _bits(g[s][want]), \
                    (b, kind, s, what)
            if want >= 0:
                scored += 1
            if pair is not None and s == 0:
                r1 = pair.acquire(np.ascontiguousarray(c.cands[b, 0]))
                assert r1.index == want, (b, kind, r1, want)
                if want >= 0:
                    assert (_bits(r1.score), _bits(r1.pdf_l), _bits(r1.pdf_g)) == \
                        (_bits(sc[want]), _bits(l[0][want]), _bits(g[0][want])), (b, kind)
        sc = _scores(l[1], g[1], F)
        wk = _topk(sc, k)
        assert top.count[b] == len(wk), (b, kind, top.count[b], len(wk))
        for j, i in enumerate(wk):
            assert top.index[b, j] == i and _bits(top.score[b, j]) == _bits(sc[i]), (b, kind, j)
            assert _bits(top.pdf_l[b, j]) == _bits(l[1][i]) and _bits(top.pdf_g[b, j]) == _bits(g[1][i]), (b, kind, j)
    return scored


@pytest.mark.parametrize("dc,du,order", CASES)
def test_records(device, monkeypatch, dc, du, order):
    c = DO.group_case(dc, du, order)
    gm = _fit(c, device)
    _check_fit(gm, c)  # the records below are checked under the oracle's models: they are the engine's too
    scored = _check_records(c, gm, monkeypatch)
    assert scored >= 3 * DO.GROUP_S  # the one-level, the signed and the plain group pick something in every pool


def test_min_bandwidth_groups(device, monkeypatch):
    """fit_groups(min_bandwidth=1e-3) on a mixed layout: the clipped bandwidths bit for bit (the constant continuous
    column's and the one-level column's among them), and the oracle's records under them."""
    from hpbandster_amd import groups
    c = DO.GroupCase(5, 2, "alternate", min_bandwidth=1e-3)
    gm = groups.fit_groups(c.X, c.losses, c.seg, c.vt, device=device, min_bandwidth=1e-3)
    assert gm.min_bandwidth == 1e-3
    _check_fit(gm, c)
    ci = c.vt.index("c")
    assert c.bw[1][0][ci] == 1e-3 and c.kinds[1] == "const_cont"  # ... now a model with finite pdfs
    assert np.isfinite(c.pdf[1][0]).any()
    _check_records(c, gm, monkeypatch)


# ---- ln-pdf ----------------------------------------------------------------------------------------------------------
_LN_REFS = {}


def _ln_refs(c):
    key = (c.dc, c.du, c.order)
    if key not in _LN_REFS:
        cat = np.array([t == "u" for t in c.vt])
        refs = {}
        for b in c.pdf:
            Xb = c.X[c.seg[b]:c.seg[b + 1]]
            for kd in (0, 1):
                bw, nl = c.bw[b][kd], c.nlev[b][kd]
                exact = bool(np.any((bw[cat] > 1.0) & (nl[cat] > 1)) or np.any(nl[cat] == 1))
                lsp = O.log_pdf_many(Xb[c.rows[b][kd]], bw, c.vt, c.cands[b, 0], nl)
                ex = c.pdf[b][kd][0]
                with np.errstate(all="ignore"):
                    refs[(b, kd)] = (exact, np.log(ex) if exact else lsp, ex, lsp)
        _LN_REFS[key] = refs
    return _LN_REFS[key]


@pytest.mark.parametrize("fp64_only", [False, True])
@pytest.mark.parametrize("dc,du,order", CASES)
def test_logpdf(device, dc, du, order, fp64_only):
    c = DO.group_case(dc, du, order)
    gm = _fit(c, device)
    r = gm.logpdf(np.ascontiguousarray(c.cands[:, 0]), fp64_only=fp64_only)
    refs = _ln_refs(c)
    for b in range(c.B):
        kind = c.kinds.get(b)
        if kind in ("no_model", "unsupported"):
            assert r.status[b] & (NO_MODEL if kind == "no_model" else UNSUPPORTED), (b, kind, r.status[b])
            assert np.all(np.isnan(r.ln_l[b])) and np.all(np.isnan(r.ln_g[b])), (b, kind)
            continue
        for kd, got in enumerate((r.ln_l[b], r.ln_g[b])):
            exact, ref, ex, lsp = refs[(b, kd)]
            tag = (dc, du, order, fp64_only, b, kind, "g" if kd else "l")
            if exact:
                assert r.status[b] & (EXACT_G if kd else EXACT_L), tag
                _check_exact(got, ref, ex, lsp, tag)
            else:
                _check_positive(got, ref, 1e-5, tag)
                ok = ex > 1e-300  # ... and ln of the exact pdf where that is a normal number
                assert np.all(np.abs(got[ok] - np.log(ex[ok])) <= 1e-5 * np.maximum(1.0, np.abs(np.log(ex[ok])))), tag


# ---- sampling and get_config ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dc,du,order", CASES)
def test_sample_and_get_config(device, dc, du, order):
    """sample: candidate (b, i) is candidate i of the single sampler on group b's good KDE at counter_base + b C, byte
    for byte, under the permuted level counts.  get_config is sample -> acquire_requests -> finish byte for byte,
    and its picks are the oracle's over the candidates it drew."""
    from hpbandster_amd import groups
    c = DO.group_case(dc, du, order)
    gm = _fit(c, device)
    B, S, C = c.B, DO.GROUP_S, DO.GROUP_C
    levels = [int(v) for v in c.levels]
    assert [v > 0 for v in levels] == [t == "u" for t in c.vt]
    base = 12345
    cands, derr = gm.sample(C, seed=9, levels=levels, bandwidth_factor=3, counter_base=base)
    ch, eh = cands.cpu().numpy(), derr.cpu().numpy()
    for b in range(B):
        kind = c.kinds.get(b)
        if kind == "no_model":
            assert np.all(np.isnan(ch[b])) and not eh[b].any()
            continue
        if kind == "unsupported":  # (no single pair can be built of it)
            continue
        c1, _, e1 = gm.pair(b).good.sample(levels, 3, C, 9, base + b * C, table=False)
        assert ch[b].tobytes() == c1.cpu().numpy().tobytes(), (b, kind)
        np.testing.assert_array_equal(eh[b], e1.cpu().numpy()[:C])
        if kind != "const_cont":
            for d, lv in enumerate(levels):  # every dim drawn as its own kind
                col = ch[b][:, d]
                if lv and kind != "signed":
                    assert np.all((col == np.floor(col)) & (col >= 0) & (col < lv)), (b, d)
                if not lv:
                    assert np.unique(col).size > C // 2, (b, d)
    seed, cb, rf = 11, 5000, 1.0 / 3
    fused = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, keep_pools=True)
    sc_, err = gm.sample(C, seed, levels, counter_base=cb, requests=S)
    rec = gm.acquire_requests(sc_, sync=False)
    comp = gm.finish(sc_, rec, err, levels, rf, seed, cb)
    assert fused.cands.tobytes() == sc_.cpu().numpy().tobytes()
    picks = groups.GroupPicks.from_bytes(rec.cpu().numpy().tobytes(), B, S)
    for name in groups.GroupPicks.__slots__:
        assert getattr(fused.picks, name).tobytes() == getattr(picks, name).tobytes(), name
    assert fused.rows.tobytes() == comp.rows.tobytes() and fused.source.tobytes() == comp.source.tobytes()
    pools = sc_.cpu().numpy()
    checked = 0
    for b in c.pdf:
        for s in range(S):
            l, g = c.pdfs_of(b, pools[b, s])
            sc = _scores(l, g, F)
            want = _argmin(sc)
            assert picks.index[b, s] == want, (b, s, picks.index[b, s], want)
            if want >= 0:
                checked += 1
                assert _bits(picks.score[b, s]) == _bits(sc[want])
                assert _bits(picks.pdf_l[b, s]) == _bits(l[want]) and _bits(picks.pdf_g[b, s]) == _bits(g[want])
                if fused.source[b, s] == SRC_MODEL:
                    assert fused.rows[b, s].tobytes() == pools[b, s, want].tobytes()
    assert checked >= 2 * S


def test_group_bohb_mixed_var_type(device):
    """GroupBOHB with var_type "ucuc": one new_results / get_configs step, every source HBX_CFG_MODEL, the model's
    bandwidths the rule's on the oracle's split."""
    from hpbandster_amd import groups
    B, m, vt, levels = 3, 14, "ucuc", [3, 0, 4, 0]
    rs = np.random.RandomState(12)
    X = rs.rand(B, m, 4)
    X[:, :, 0] = rs.randint(0, 3, size=(B, m))
    X[:, :, 2] = rs.randint(0, 4, size=(B, m))
    losses = rs.rand(B, m)
    opt = groups.GroupBOHB(B, vt, levels, num_samples=32, random_fraction=0.0, seed=5, device=device)
    assert opt.new_results(9.0, X, losses)
    cfg = opt.get_configs(9.0, S=2)
    assert np.all(cfg.source == SRC_MODEL), cfg.source
    gm = opt.kde_models[9.0]
    bwg, bwb = gm.bandwidths()
    for b in range(B):
        g_rows, b_rows = DO.group_split(losses[b], 4)
        assert bwg[b].tobytes() == O.normal_reference_bw(X[b][g_rows]).tobytes()
        assert bwb[b].tobytes() == O.normal_reference_bw(X[b][b_rows]).tobytes()
    rows = np.asarray(cfg.rows).reshape(B, 2, 4)
    for d, lv in enumerate(levels):
        col = rows[:, :, d]
        assert np.all((col == np.floor(col)) & (col >= 0) & (col < lv)) if lv else np.all(col != np.floor(col)), d
