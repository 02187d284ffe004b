"""Grouped ln-pdf, the signed log-space route (HBX_LOGPDF_SIGNED, GroupModel.logpdf(signed="logspace")) on the GPU:
KDEs with a categorical bandwidth > 1 against the fp64 signed log-space oracle where the signed sum is well
conditioned, and against the same call's exact route everywhere else.
"""
import functools

import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import SHAPES, _groups

pytestmark = pytest.mark.gpu

EXACT, SIGNED = (64, 128), (256, 512)
CASES = [s for s in SHAPES if s[1]] + [(40, 6)]  # (40, 6): the 64 + 32-slot bucket, two waves per block
ROUNDS = [0, 76, 77, 151, 152]  # + D + 2: n_bad = 64, 65 (one round of 2 waves, + 1) and 128, 129 (of 4 waves, + 1)


@functools.lru_cache(maxsize=None)
def _case(device, dc, du, C, src):
    """src "ragged": test_gpu_groups' groups; "rounds": groups of ROUNDS rows, 12 levels (every bandwidth > 1), half of
    each pool on or near observation rows.  Fitted once; per signed-only KDE -- grp_classify's rule on the host -- the
    references: sig[(b, kd)] = (lsp, well), `well`: kappa = (S+ + S-) / |S+ - S-| <= 1e3 and S+ > S-."""
    from hpbandster_amd import groups
    D = dc + du
    if src == "ragged":
        X, losses, seg, vt, _, cands, _ = _groups(dc, du, C)
    else:
        rs = np.random.RandomState(7 * D + C)
        seg = np.concatenate([[0], np.cumsum(np.array(ROUNDS) + [D + 2, 0, 0, 0, 0])]).astype(np.int64)
        n, vt = int(seg[-1]), "c" * dc + "u" * du
        X = np.hstack([rs.rand(n, dc), rs.randint(0, 12, size=(n, du)).astype(np.float64)])
        losses = rs.rand(n)
        cands = np.hstack([rs.rand(len(ROUNDS) * C, dc), rs.randint(0, 12, size=(len(ROUNDS) * C, du))]).reshape(-1, C, D)
        for b in range(len(ROUNDS)):
            cands[b, :(C + 1) // 2] = X[seg[b]:seg[b + 1]][rs.randint(0, seg[b + 1] - seg[b], size=(C + 1) // 2)]
            cands[b, :(C + 3) // 4, :dc] += 0.01 * rs.randn((C + 3) // 4, dc)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    cat = np.arange(D) >= dc
    bws, nls = gm.bandwidths(), (gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy())
    sig = {}
    for b in np.flatnonzero(gm.has_model):
        # With several h > 1 dims the sign of a term is the parity of its matches there, and at a pool drawn like the
        # rows about half the sums are negative (the reference's pdf is NaN).  Six in seven candidates get a level
        # that no row has in those dims (every term positive); the seventh keeps its codes: sums of both signs.
        with np.errstate(invalid="ignore"):
            cands[b][np.ix_(np.arange(C) % 7 != 6, cat & ((bws[0][b] > 1.0) | (bws[1][b] > 1.0)))] = 1000.0
        for kd, rows in enumerate(gm.rows_of(b)):
            bw, nl, data = bws[kd][b], nls[kd][b], X[seg[b]:seg[b + 1]][rows]
            if not (np.any(bw[cat] > 1.0) and np.all(nl[cat] >= 2) and np.all((bw[~cat] > 0) & np.isfinite(bw[~cat]))):
                continue
            m = cands[b][:, None, dc:] == data[None, :, dc:]  # the signed terms, as kde_oracle.log_pdf_many forms them
            with np.errstate(divide="ignore"):
                logk = np.where(m, np.log(np.abs(1 - bw[cat])), np.log(bw[cat] / (nl[cat] - 1))).sum(-1) - \
                    (((cands[b][:, None, :dc] - data[None, :, :dc]) / bw[:dc]) ** 2).sum(-1) / 2
            e = np.exp(logk - logk.max(1, keepdims=True)) * (1 - 2 * ((m & (bw[cat] > 1)).sum(-1) & 1))
            with np.errstate(all="ignore"):
                well = (e.sum(1) > 0) & (np.abs(e).sum(1) <= 1e3 * e.sum(1))
            sig[(b, kd)] = (O.log_pdf_many(data, bw, vt, cands[b], nl), well)
    return dict(gm=gm, cands=cands, sig=sig)


@functools.lru_cache(maxsize=None)
def _run(device, dc, du, C, src, fp64_only, signed):
    case = _case(device, dc, du, C, src)
    return case["gm"].logpdf(case["cands"], fp64_only=fp64_only, signed=signed)


@pytest.mark.parametrize("fp64_only", [False, True])
@pytest.mark.parametrize("src", ["ragged", "rounds"])
@pytest.mark.parametrize("C", [1, 70])
@pytest.mark.parametrize("dc,du", CASES)
def test_contract_on_the_signed_route(device, dc, du, C, src, fp64_only):
    """Well-conditioned candidates of the signed KDEs, by the oracle alone (checked on the CPU with the oracle's
    normal-reference bandwidths): C = 1: 100 % in every case; C = 70, ragged: 99.6, 98.3, 93.7, 92.8 % for (0, 3),
    (5, 2), (24, 8), (40, 6), rounds: 92.7, 96.8, 93.6, 95.5 %.  No candidate with kappa > 1e3 has an |ln p| large
    enough for the pass's bound to accept it."""
    case = _case(device, dc, du, C, src)
    r, ex = _run(device, dc, du, C, src, fp64_only, "logspace"), _run(device, dc, du, C, src, fp64_only, "exact")
    assert case["sig"] and sum(r.stats) == 2 * len(r) * C
    nwell = 0
    for (b, kd), (lsp, well) in case["sig"].items():
        assert r.status[b] & SIGNED[kd] and not r.status[b] & EXACT[kd], (b, kd, r.status[b])
        assert ex.status[b] & EXACT[kd] and not ex.status[b] & SIGNED[kd], (b, kd, ex.status[b])
        got, want = (r.ln_g if kd else r.ln_l)[b], (ex.ln_g if kd else ex.ln_l)[b]
        err = np.abs(got[well] - lsp[well]) / np.maximum(1.0, np.abs(lsp[well]))
        print("(%d, %d) C = %d %s group %d KDE %d: %d of %d well conditioned, max error %.3g"
              % (dc, du, C, src, b, kd, well.sum(), C, err.max(initial=0.0)))
        assert np.all(err <= 1e-5), (b, kd, err.max())
        assert np.array_equal(got[~well], want[~well], equal_nan=True), (b, kd, got[~well], want[~well])
        nwell += int(well.sum())
    assert nwell >= 0.9 * C * len(case["sig"]), (nwell, C * len(case["sig"]))
    assert r.stats[1] > 0 and r.stats[2] <= ex.stats[2] and r.stats[3] == ex.stats[3]


@pytest.mark.parametrize("fp64_only", [False, True])
def test_cancelling_sums_are_handed_to_the_exact_path(device, fp64_only):
    """One categorical dim with h > 1, every row but one at level 0, the candidates at level 0 beside the rows: every
    dominant term is negative, the reference's pdf is negative, the value NaN on both routes."""
    from hpbandster_amd import groups
    rs = np.random.RandomState(5)
    n, C = 40, 70
    X = np.hstack([rs.rand(n, 2), np.zeros((n, 1))])
    X[n - 1, 2] = 30.0  # the worst row, so in the bad KDE (34 rows): h = 1.06 * 5.07 * 34^(-1/7) = 3.2, two levels
    gm = groups.fit_groups(X, np.arange(n, dtype=np.float64), np.array([0, n]), "ccu", device=device)
    assert gm.bandwidths()[1][0][2] > 1.0 and gm.nlev_bad.cpu().numpy()[0][2] == 2
    cands = np.hstack([X[rs.randint(0, n - 1, size=C), :2] + 0.01 * rs.randn(C, 2), np.zeros((C, 1))])[None]
    r, ex = (gm.logpdf(cands, fp64_only=fp64_only, signed=s) for s in ("logspace", "exact"))
    assert r.status[0] & SIGNED[1] and ex.status[0] & EXACT[1]
    assert np.all(np.isnan(ex.ln_g)) and r.stats[2] > 0
    np.testing.assert_array_equal(np.isnan(r.ln_g), np.isnan(ex.ln_g))
    assert r.ln_l.tobytes() == ex.ln_l.tobytes()


def test_ranking_on_the_signed_route(device):
    dc, du, C, k = 5, 2, 70, 4
    case = _case(device, dc, du, C, "ragged")
    gm, cands = case["gm"], case["cands"]
    lp = _run(device, dc, du, C, "ragged", True, "logspace")
    rk, dflt, old = gm.rank_logratio(cands, k, signed="logspace"), gm.rank_logratio(cands, k), gm.rank_logratio(
        cands, k, signed="exact")
    assert dflt.index.tobytes() == old.index.tobytes() and dflt.score.tobytes() == old.score.tobytes()
    np.testing.assert_array_equal(rk.status, lp.status)
    assert np.any(rk.status & (SIGNED[0] | SIGNED[1])) and not np.any(dflt.status & (SIGNED[0] | SIGNED[1]))
    for b in range(len(lp)):
        with np.errstate(invalid="ignore"):
            s = lp.ln_g[b] - lp.ln_l[b]
        order = [i for i in np.lexsort((np.arange(C), s + 0.0)) if not np.isnan(s[i])][:k]  # (+ 0.0: -0 as +0)
        assert rk.count[b] == len(order), b
        assert rk.index[b, :len(order)].tobytes() == np.array(order, np.int32).tobytes(), b
        assert rk.score[b, :len(order)].tobytes() == s[order].tobytes(), b
        if not rk.status[b] & (SIGNED[0] | SIGNED[1]):  # no signed KDE: the default call's result, unchanged
            assert rk.index[b].tobytes() == dflt.index[b].tobytes() and rk.score[b].tobytes() == dflt.score[b].tobytes()


def test_default_route_is_unchanged(device):
    dc, du, C = 5, 2, 70
    case = _case(device, dc, du, C, "ragged")
    a, b = case["gm"].logpdf(case["cands"]), _run(device, dc, du, C, "ragged", True, "exact")
    assert a.ln_l.tobytes() == b.ln_l.tobytes() and a.ln_g.tobytes() == b.ln_g.tobytes()
    assert a.status.tobytes() == b.status.tobytes() and a.stats == b.stats
    assert not np.any(a.status & (SIGNED[0] | SIGNED[1]))
