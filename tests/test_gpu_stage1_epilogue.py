"""Stage 1 of the staged single acquisition with lhi and the block maxima from the scoring kernel's epilogue
(hbx_score_h32.hip, hbx_staged.hip): where the good KDE's launch runs unsplit, the coarse pair kernel leaves every
candidate's l bound and one maximum per block, staged_l_kernel is not launched, and the seed kernel reduces the
maxima and re-scores the candidates stage 1 rescue-marked.  HBX_STAGE1_LHI=0 launches staged_l_kernel as before.

Every case runs the same pair, candidates and workspace with HBX_STAGED=2 and HBX_STAGE1_LHI unset and =0, the fold
before and after the launch of its own: every record field, hbx_kde_acquire_stats and the Lmax word must be equal
(the one exception, rescue-marked l estimates, says so), and KDEPair.acquire_stage1 proves which branch ran.  Both
coarse pair kernels are covered: the one-tile kernel these small launches take by themselves, and, with HBX_PAIR1=0,
the two-tile kernel of large launches.  Pairs are bench-like, 24c + 8u with 4 levels, fitted by
tests/test_gpu_staged.py's recipe (BOHB's split, normal-reference bandwidths, categorical ones capped at 0.8), both
KDEs on the coarse <3, 1> instance.
"""
import struct

import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

NEG_INF_BITS = 0x007FFFFF  # hbx_f2ord(-inf): the Lmax word when no candidate contributes


def _fit(X, losses, vt, device, cat_bw=0.8, bw_good=None, bw_bad=None):
    from hpbandster_amd import kde
    g_idx, b_idx = O.bohb_split(X, losses, X.shape[1] + 1)
    cat = np.array([v == "u" for v in vt])
    with np.errstate(all="ignore"):
        bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    bwg[cat] = np.minimum(bwg[cat], cat_bw)
    bwb[cat] = np.minimum(bwb[cat], cat_bw)
    if bw_good is not None:
        bwg = bw_good(bwg)
    if bw_bad is not None:
        bwb = bw_bad(bwb)
    nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, nlg, nlb, device=device)
    assert (pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1  # both on the coarse 32x32 instance
    return pair


def _record(r):
    """Every field of a record, NaN-safe."""
    return (r.index, struct.pack("<ddd", r.score, r.pdf_l, r.pdf_g), r.flags, r.near, struct.pack("<f", r.rel),
            r.shortlist)


def _same(on, off):
    """tests/test_gpu_staged.py's rule for a staged record against the unstaged one."""
    assert on.index == off.index, (on, off)
    assert struct.pack("<ddd", on.score, on.pdf_l, on.pdf_g) == struct.pack("<ddd", off.score, off.pdf_l, off.pdf_g)
    assert (on.flags, on.near) == (off.flags, off.near), (on, off)
    assert struct.pack("<f", on.rel) == struct.pack("<f", off.rel), (on, off)
    assert on.shortlist in (off.shortlist, off.shortlist - 1), (on.shortlist, off.shortlist)


def _oracle_pick(pair, vt, C):
    from oracle import c_oracle
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    return O.select(l, g)[0]


def _run(pair, Cd, ws, monkeypatch, fold, expect_fold=None):
    """One staged call: (record, stats, Lmax word); asserts which branch left lhi."""
    if fold:
        monkeypatch.delenv("HBX_STAGE1_LHI", raising=False)
    else:
        monkeypatch.setenv("HBX_STAGE1_LHI", "0")
    rec = pair.acquire(Cd, workspace=ws)
    st = pair.acquire_stats(ws, len(Cd))
    s1 = pair.acquire_stage1(ws, len(Cd))
    assert st["staged"], st
    assert s1["lhi_epilogue"] == (fold if expect_fold is None else expect_fold), (fold, s1)
    return rec, st, s1["lmax_bits"]


def _ab(pair, C, monkeypatch, device, pair1=True, seeds_may_differ=False):
    """The fold's (record, stats, Lmax word), equal to the separate launch's on the same workspace -- run before it
    and after it, so either form also starts from the state the other one left."""
    import torch
    monkeypatch.setenv("HBX_STAGED", "2")
    if pair1:
        monkeypatch.delenv("HBX_PAIR1", raising=False)
    else:
        monkeypatch.setenv("HBX_PAIR1", "0")
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    on0, st_on0, lm_on0 = _run(pair, Cd, ws, monkeypatch, True)
    off, st_off, lm_off = _run(pair, Cd, ws, monkeypatch, False)
    on, st_on, lm_on = _run(pair, Cd, ws, monkeypatch, True)
    print("fold off", off, st_off, hex(lm_off), "fold on", on, st_on, hex(lm_on))
    assert _record(on0) == _record(on) and st_on0 == st_on and lm_on0 == lm_on, (on0, on, st_on0, st_on)
    if seeds_may_differ:
        _same(on, off)
    else:
        assert _record(on) == _record(off), (on, off)
        assert st_on == st_off, (st_on, st_off)
        assert lm_on == lm_off, (hex(lm_on), hex(lm_off))
    return on, st_on, lm_on, off, st_off, lm_off, Cd, ws


def _unstaged(pair, Cd, ws, monkeypatch):
    monkeypatch.setenv("HBX_STAGED", "0")
    rec = pair.acquire(Cd, workspace=ws)
    assert not pair.acquire_stats(ws, len(Cd))["staged"]
    assert not pair.acquire_stage1(ws, len(Cd))["lhi_epilogue"]
    return rec


@pytest.fixture(scope="module")
def bench_like(device):
    """tests/test_gpu_staged.py's: 24c + 8u with 4 levels, 400 observations (60 good: one chunk, so stage 1 runs
    unsplit), 4099 candidates."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=211)
    pair = _fit(X, S.make_losses(400, seed=212), vt, device)
    C = S.make_candidates(4099, 24, 8, 4, seed=213)
    return pair, vt, C


@pytest.mark.parametrize("pair1", [True, False], ids=["one_tile", "two_tiles"])
@pytest.mark.parametrize("nc", [1, 31, 33, 63, 65, 511, 512, 513, 1025, 4099])
def test_same_result_fold_on_and_off(device, monkeypatch, bench_like, nc, pair1):
    """Partly filled column tiles, waves and blocks, and a last block with a single candidate, in front of the block
    maximum; with HBX_PAIR1=0 the two-tile kernel, whose lane half 1 finishes the second tile."""
    pair, vt, C = bench_like
    on, st, lm, *_ = _ab(pair, C[:nc], monkeypatch, device, pair1=pair1)
    assert 0 <= on.index < nc and 1 <= st["evaluated"] <= nc
    assert lm > NEG_INF_BITS  # some candidate has a finite lower l bound


def test_seed_kernel_tile_loop(device, monkeypatch, bench_like):
    """More than 2048 x 1024 candidates: behind the fold the seed kernel's grid stops at 2048 blocks (each reads
    every block maximum) and its blocks walk the 1024-candidate tiles in a loop, a last partly filled one among
    them; the separate launch's seed kernel keeps a block per tile.  Candidates are drawn on the device."""
    import torch
    pair, vt, C = bench_like
    nc = 2048 * 1024 + 2 * 1024 + 7
    gen = torch.Generator(device=device).manual_seed(713)
    Cd = torch.rand(nc, 32, dtype=torch.float64, device=device, generator=gen)
    Cd[:, 24:] = torch.randint(0, 4, (nc, 8), device=device, generator=gen).to(torch.float64)
    Cd[nc - 3] = torch.from_numpy(C[3089]).to(device)  # the 4099's winner, in the last tile
    monkeypatch.setenv("HBX_STAGED", "2")
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)
    on0, st_on0, lm_on0 = _run(pair, Cd, ws, monkeypatch, True)
    off, st_off, lm_off = _run(pair, Cd, ws, monkeypatch, False)
    on, st_on, lm_on = _run(pair, Cd, ws, monkeypatch, True)
    print("fold off", off, st_off, "fold on", on, st_on)
    assert _record(on0) == _record(on) == _record(off)
    assert st_on0 == st_on == st_off and lm_on0 == lm_on == lm_off
    assert 1 <= st_on["seeds"] < 4096 and on.index >= 0


def test_pick_is_the_oracles(device, monkeypatch, bench_like):
    pair, vt, C = bench_like
    on, st, lm, off, st_off, lm_off, Cd, ws = _ab(pair, C, monkeypatch, device)
    _same(on, _unstaged(pair, Cd, ws, monkeypatch))
    assert on.index == _oracle_pick(pair, vt, C)


def test_split_stage_one_falls_back(device, monkeypatch):
    """1e4 observations (1500 good: 24 chunks) and 700 candidates: pair_shape splits the good KDE's observations, the
    partial sums need staged_l_kernel's merge, so the fold is off whatever the switch says."""
    import torch
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(10000, 24, 8, 4, seed=511)
    pair = _fit(X, S.make_losses(10000, seed=512), vt, device)
    C = S.make_candidates(700, 24, 8, 4, seed=513)
    monkeypatch.setenv("HBX_STAGED", "2")
    Cd = torch.from_numpy(C).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    a, st_a, lm_a = _run(pair, Cd, ws, monkeypatch, True, expect_fold=False)
    b, st_b, lm_b = _run(pair, Cd, ws, monkeypatch, False)
    assert _record(a) == _record(b) and st_a == st_b and lm_a == lm_b
    _same(a, _unstaged(pair, Cd, ws, monkeypatch))
    monkeypatch.setenv("HBX_STAGED", "2")
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")  # the same launch unsplit: the fold is back
    c, st_c, lm_c = _run(pair, Cd, ws, monkeypatch, True)
    assert c.index == a.index and _record(c)[1] == _record(a)[1]


@pytest.mark.parametrize("pair1", [True, False], ids=["one_tile", "two_tiles"])
def test_rescue_markers_every_l(device, monkeypatch, pair1):
    """tests/test_gpu_staged.py's test_rescue_markers_among_the_seeds, turned on the good KDE: narrow in dim 0
    (bandwidth 0.004) with every candidate at x_0 = 1.6, outside the observations' [0, 1).  The probe's maximum over
    the chunk is about 2 x' X' - X'^2 in dim 0 alone (x' = s (1.6 - mean), X' = s (max - mean), s = 0.849 / 0.004),
    beyond the 30000 of the shifted c_i's three f16 pieces: every l estimate of stage 1 is a rescue marker, the
    candidate with the largest l among them.  The fold leaves +inf for each and no block maximum, so Lmax is -inf and
    the seed kernel re-scores every candidate.  A re-scored estimate at |c_i| of 5e4 has a relative bound above 1,
    a lower end of -inf: staged_l_kernel's Lmax is -inf as well and both forms seed every candidate.  The seed
    count is not compared (it may differ wherever l estimates are marked, and only there: the next test); the
    record equals the unstaged one's by the _same rule, and the pick is the C oracle's."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=261)

    def narrow(bw):
        bw = bw.copy()
        bw[0] = 0.004
        return bw
    pair = _fit(X, S.make_losses(400, seed=262), vt, device, bw_good=narrow)
    C = S.make_candidates(1300, 24, 8, 4, seed=263)
    C[:, 0] = 1.6
    g0 = np.asarray(pair.good.data)[:, 0]
    s = np.sqrt(np.log2(np.e) / 2) / 0.004
    xq, Xq = s * (1.6 - g0.mean()), s * (g0.max() - g0.mean())
    assert 2 * xq * Xq - Xq * Xq > 33000.0  # the premise: the shifted c_i is out of range for every candidate
    on, st_on, lm_on, off, st_off, lm_off, Cd, ws = _ab(pair, C, monkeypatch, device, pair1=pair1,
                                                         seeds_may_differ=True)
    print("seeds: fold", st_on["seeds"], "separate launch", st_off["seeds"])
    assert lm_on == NEG_INF_BITS  # no unmarked candidate
    assert st_on["seeds"] == len(C) >= st_off["seeds"] >= 1  # the threshold is -inf: every re-scored candidate
    ref = _unstaged(pair, Cd, ws, monkeypatch)
    _same(on, ref)
    _same(off, ref)
    assert on.index == _oracle_pick(pair, vt, C)


@pytest.mark.parametrize("pair1", [True, False], ids=["one_tile", "two_tiles"])
def test_rescue_markers_hold_the_largest_l(device, monkeypatch, pair1):
    """Marked and unmarked l estimates in one call, the largest l among the marked: the good KDE's continuous
    bandwidths scaled by 0.35, 600 observations (90 good: two chunks), one launch per KDE unsplit (HBX_OBS_SPLIT=0).  A
    candidate that IS a good observation of the second chunk and lies more than 110 log2 units from every
    observation of the first has a sum beyond 2^100 times the first chunk's largest term: a rescue marker, with
    l as large as l gets.  The other candidates are ordinary.  The fold's Lmax is the largest lower bound of the
    unmarked ones, below the separate launch's; the seed sets differ accordingly, the records do not."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(600, 24, 8, 4, seed=611)

    def narrow(bw):
        bw = bw.copy()
        bw[:24] *= 0.35
        return bw
    pair = _fit(X, S.make_losses(600, seed=612), vt, device, bw_good=narrow)
    G = np.asarray(pair.good.data)
    assert len(G) > 64
    h = np.asarray(pair.good.bw)[:24]
    late = G[64:]
    d2 = 0.5 * np.log2(np.e) * (((late[:, None, :24] - G[None, :64, :24]) / h) ** 2).sum(axis=2)
    marked = late[d2.min(axis=1) > 110.0]
    assert len(marked) >= 3, len(marked)  # the premise: markers occur
    C = S.make_candidates(1100, 24, 8, 4, seed=613)
    pos = np.linspace(5, 1090, len(marked)).astype(int)
    C[pos] = marked
    monkeypatch.setenv("HBX_OBS_SPLIT", "0")
    on, st_on, lm_on, off, st_off, lm_off, Cd, ws = _ab(pair, C, monkeypatch, device, pair1=pair1,
                                                         seeds_may_differ=True)
    print("seeds: fold", st_on["seeds"], "separate launch", st_off["seeds"])
    assert NEG_INF_BITS < lm_on < lm_off  # the largest lower bound belongs to a marked candidate
    assert st_on["seeds"] >= st_off["seeds"] >= 1  # a lower Lmax can only add seeds
    ref = _unstaged(pair, Cd, ws, monkeypatch)
    _same(on, ref)
    _same(off, ref)
    assert on.index == _oracle_pick(pair, vt, C)


@pytest.mark.parametrize("pair1", [True, False], ids=["one_tile", "two_tiles"])
def test_nan_l_for_whole_blocks(device, monkeypatch, pair1):
    """tests/test_gpu_staged.py's test_nan_l_single_level_dim: the good KDE's first categorical dim holds one
    observed level, l is NaN for every candidate without it.  Here the first 1024 candidates (two or four whole
    blocks) and the last 30 (the last block's every candidate) are off that level: those blocks' maxima are -inf,
    their candidates are never seeded and never survive."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=241)
    losses = S.make_losses(400, seed=242)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 24] = 2.0
    pair = _fit(X, losses, vt, device)
    assert pair.good.nlev[24] == 1
    C = S.make_candidates(2078, 24, 8, 4, seed=243)
    C[:, 24] = 2.0
    C[:1024, 24] = 1.0
    C[2048:, 24] = 3.0
    on, st, lm, off, st_off, lm_off, Cd, ws = _ab(pair, C, monkeypatch, device, pair1=pair1)
    assert lm > NEG_INF_BITS and 1024 <= on.index < 2048
    assert st["seeds"] + st["survivors"] <= 1024
    _same(on, _unstaged(pair, Cd, ws, monkeypatch))
    assert on.index == _oracle_pick(pair, vt, C)


def test_nan_l_everywhere(device, monkeypatch):
    """tests/test_gpu_staged.py's: a constant continuous column in the good rows (`nan_all`), l NaN for every
    candidate.  Every block maximum is -inf, Lmax stays -inf, nothing is seeded, nothing survives, index -1."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=251)
    losses = S.make_losses(400, seed=252)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 5] = 0.25
    pair = _fit(X, losses, vt, device)
    assert pair.good.bw[5] == 0
    C = S.make_candidates(1500, 24, 8, 4, seed=253)
    on, st, lm, off, st_off, lm_off, Cd, ws = _ab(pair, C, monkeypatch, device)
    assert lm == NEG_INF_BITS and on.index == -1
    assert (st["seeds"], st["survivors"], st["evaluated"]) == (0, 0, 0), st
    _same(on, _unstaged(pair, Cd, ws, monkeypatch))


def test_staged_topk_untouched(device, monkeypatch, bench_like):
    """The staged top-k wants every candidate's key of -llo from staged_l_kernel: it runs that launch whatever the
    switch says, and its output is the same bytes."""
    import torch
    pair, vt, C = bench_like
    k, nc = 8, 2049
    monkeypatch.setenv("HBX_STAGED", "2")
    Cd = torch.from_numpy(np.ascontiguousarray(C[:nc])).to(device)
    ws = torch.empty(pair.topk_workspace_bytes(nc, k), dtype=torch.uint8, device=device)
    out = []
    for sw in (None, "0", None):
        if sw is None:
            monkeypatch.delenv("HBX_STAGE1_LHI", raising=False)
        else:
            monkeypatch.setenv("HBX_STAGE1_LHI", sw)
        r = pair.acquire_topk(Cd, k, workspace=ws)
        assert pair.acquire_stats(ws, nc)["staged"]
        assert not pair.acquire_stage1(ws, nc)["lhi_epilogue"]
        out.append((r.count, r.flags, r.shortlist) + tuple(getattr(r, f).tobytes()
                                                            for f in ("index", "score", "pdf_l", "pdf_g", "rel")))
    assert out[0] == out[1] == out[2]
