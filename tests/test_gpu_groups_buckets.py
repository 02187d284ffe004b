"""The grouped calls at the slot buckets and code paths the other grouped tests never reach through acquire,
acquire_requests and acquire_topk (their shapes stop at D = 32 with at most 8 categorical dims): the 16-slot and the
64 + 32-slot instances, the pair loop with a uniform branch per piece, the second staging round (dims past 64) and
the bucket-overflow rule.  Per shape: every record of acquire and of acquire_requests (S = 3, under either screen)
equals the oracle's (c_oracle.kde_pdf(exact=True) + kde_oracle.select) in index, score and both pdfs bit for bit, the
top-5 equals the oracle's ranking, and both ln pdfs are within 1e-5 of the log-space oracle in both modes.  The screens
must also do their work: a shape whose groups fit the bucket certifies something (the shortlists together are
shorter than the pools, the ln-pdf's fp32 pass writes values); the shape past the bucket re-scores everything.

The fixture is test_gpu_groups_logpdf.py::test_unsigned_categorical_buckets' construction (hpbandster_amd.synthetic;
few levels keep every categorical bandwidth below 1): three groups of D + 2, max(D + 2, 70) and 200 rows -- one
partial chunk, a second wave's rows, and every wave of the tile screen busy with two 128-row chunks -- and pools of
C = 65 candidates (two tiles, the second with one live lane), half of each pool observation rows or within 0.01 of
one, a tenth far (4 + rand), the rest uniform, as test_gpu_groups.py::_groups mixes them.  No input had to be changed
for the two screening conditions: they hold at every shape as built.

The shape past the bucket (70 continuous dims): every KDE goes through ln of the reference's own fp64 pdf, which is
0 (-inf) for the far candidates where the log-space oracle is finite.  Its values are therefore checked as the exact
KDEs of test_gpu_groups_logpdf.py are (_check_exact, 1e-12 against ln of the exact pdf), and against the log-space
oracle at 1e-5 wherever the exact pdf is a normal number.
"""
import functools

import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import OVERFLOW, _oracle, _same
from tests.test_gpu_groups_logpdf import EXACT_G, EXACT_L, _check_exact, _check_positive
from tests.test_gpu_groups_topk import _check_block, _ranked

pytestmark = pytest.mark.gpu

# (dc, du, levels): 16 slots, 4 + 2 compile-time pieces | more than 8 categorical dims: the uniform-branch loop |
# 32 slots, 6 pieces, no categorical dim | 64 + 32 slots, two waves, more than 32 continuous dims | D = 68: the second
# staging round | more continuous dims than the bucket holds: every group exact-only
SHAPES = [(12, 3, 2), (3, 10, 2), (20, 0, 2), (40, 6, 3), (60, 8, 2), (70, 4, 2)]
PAST_THE_BUCKET = (70, 4, 2)
S_REQ, C, K = 3, 65, 5


@functools.lru_cache(maxsize=None)
def _case(device, dc, du, lev):
    """The fitted groups, the S_REQ pools per group and the oracle's pdfs of every pool, computed once per shape and
    never changed.  acquire, acquire_topk and logpdf take request 0's pools."""
    from hpbandster_amd import groups
    from hpbandster_amd import synthetic as S
    D = dc + du
    lens = np.array([D + 2, max(D + 2, 70), 200])
    B = len(lens)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = S.make_observations(int(seg[-1]), dc, du, lev, seed=41)
    losses = S.make_losses(int(seg[-1]), seed=42)
    vt = S.var_type_string(dc, du)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    rs = np.random.RandomState(43)
    P = S_REQ * C
    cands = S.make_candidates(B * P, dc, du, lev, seed=44).reshape(B, P, D)
    for b in range(B):
        k = rs.rand(P)
        src = X[seg[b]:seg[b + 1]][rs.randint(0, lens[b], size=P)]
        cands[b, k < 0.25] = src[k < 0.25]  # observation rows as candidates
        pt = (k >= 0.25) & (k < 0.5)
        cands[b, pt] = src[pt]
        cands[b, pt, :dc] += 0.01 * rs.randn(int(pt.sum()), dc)
        far = (k >= 0.5) & (k < 0.6)
        cands[b, far, :dc] = 4.0 + rs.rand(int(far.sum()), dc)  # pdfs underflow to 0
    cands = np.ascontiguousarray(cands.reshape(B, S_REQ, C, D))
    ora = {(b, s): _oracle(gm, X, seg, vt, cands[:, s], b) for b in range(B) for s in range(S_REQ)}
    return dict(gm=gm, X=X, seg=seg, vt=vt, cands=cands, ora=ora, B=B, pool0=np.ascontiguousarray(cands[:, 0]))


def _check_record(rec, l, g, where):
    want, scores = O.select(l, g)
    assert rec[0] == want, (where, rec, want)
    if want >= 0:
        assert _same(rec[2], l[want]) and _same(rec[3], g[want]) and rec[1] == scores[want], (where, rec)
    else:
        assert all(np.isnan(v) for v in rec[1:]), (where, rec)


def _check_screening(shape, flags, shortlist, pools, what):
    """past the bucket: OVERFLOW and every candidate re-scored; inside it: the screen certifies something"""
    print("%s %s: shortlists %s of %d" % (shape, what, shortlist.reshape(-1).tolist(), C))
    if shape == PAST_THE_BUCKET:
        assert np.all(flags & OVERFLOW) and np.all(shortlist == C), (shape, what, flags, shortlist)
    else:
        assert not np.any(flags & OVERFLOW), (shape, what, flags)
        assert shortlist.sum() < pools * C, (shape, what, shortlist)


@pytest.mark.parametrize("dc,du,lev", SHAPES)
def test_acquire_equals_the_oracle(device, dc, du, lev):
    case = _case(device, dc, du, lev)
    picks = case["gm"].acquire(case["pool0"])
    assert len(picks) == case["B"]
    for b in range(case["B"]):
        l, g = case["ora"][(b, 0)]
        _check_record((picks.index[b], picks.score[b], picks.pdf_l[b], picks.pdf_g[b]), l, g, (dc, du, b))
    _check_screening((dc, du, lev), picks.flags, picks.shortlist, case["B"], "acquire")


@pytest.mark.parametrize("screen", ["1", "2"])
@pytest.mark.parametrize("dc,du,lev", SHAPES)
def test_requests_equal_the_oracle_under_either_screen(device, monkeypatch, dc, du, lev, screen):
    monkeypatch.setenv("HBX_GROUPS_SCREEN", screen)
    case = _case(device, dc, du, lev)
    picks = case["gm"].acquire_requests(case["cands"])
    assert picks.index.shape == (case["B"], S_REQ)
    for b in range(case["B"]):
        for s in range(S_REQ):
            l, g = case["ora"][(b, s)]
            _check_record((picks.index[b, s], picks.score[b, s], picks.pdf_l[b, s], picks.pdf_g[b, s]), l, g,
                          (dc, du, screen, b, s))
    for s in range(S_REQ):
        _check_screening((dc, du, lev), picks.flags[:, s], picks.shortlist[:, s], case["B"],
                         "screen %s request %d" % (screen, s))


@pytest.mark.parametrize("dc,du,lev", SHAPES)
def test_topk_equals_the_oracles_ranking(device, dc, du, lev):
    case = _case(device, dc, du, lev)
    top = case["gm"].acquire_topk(case["pool0"], K)
    assert len(top) == case["B"] and top.k == K
    for b in range(case["B"]):
        l, g = case["ora"][(b, 0)]
        _check_block(top, b, (l, g) + _ranked(l, g), K, (dc, du))
    _check_screening((dc, du, lev), top.flags, top.shortlist, case["B"], "top-k")


@pytest.mark.parametrize("dc,du,lev", SHAPES)
def test_logpdf_within_rtol_in_both_modes(device, dc, du, lev):
    case = _case(device, dc, du, lev)
    gm, X, seg, vt, pool, B = case["gm"], case["X"], case["seg"], case["vt"], case["pool0"], case["B"]
    bws = gm.bandwidths()
    nls = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    past = (dc, du, lev) == PAST_THE_BUCKET
    runs = [gm.logpdf(pool, fp64_only=False), gm.logpdf(pool, fp64_only=True)]
    print("stats (%d, %d): default %s, fp64 only %s" % (dc, du, runs[0].stats, runs[1].stats))
    for mode, r in enumerate(runs):
        assert sum(r.stats) == 2 * B * C and r.stats[3] == 0
        if past:
            assert np.all(r.status == (EXACT_L | EXACT_G)), r.status
            assert r.stats[2] == 2 * C * B
        else:
            assert np.all(r.status == 0), r.status
            assert r.stats[2] == 0
        for b in range(B):
            Xb = X[seg[b]:seg[b + 1]]
            for kd, rows in enumerate(gm.rows_of(b)):
                got = (r.ln_g if kd else r.ln_l)[b]
                tag = (dc, du, mode, b, kd)
                lsp = O.log_pdf_many(Xb[rows], bws[kd][b], vt, pool[b], nls[kd][b])
                if not past:
                    _check_positive(got, lsp, 1e-5, tag)
                    continue
                ex = case["ora"][(b, 0)][kd]  # the reference's own fp64 pdf
                with np.errstate(all="ignore"):
                    _check_exact(got, np.log(ex), ex, lsp, tag)
                normal = ex > 1e-300
                assert normal.any(), tag
                _check_positive(got[normal], lsp[normal], 1e-5, tag)
    assert runs[1].stats[0] == 0
    if not past:
        assert runs[0].stats[0] > 0  # the fp32 pass certifies something
