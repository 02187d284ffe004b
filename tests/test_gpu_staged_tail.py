"""The short tail of the staged single acquisition (hbx_staged.hip, HBX_STAGED_TAIL): the survivor pass leaves the
pruned candidates' l-only bounds, staged_tail_kernel merges the survivors' partials and takes the evaluated
candidates' score intervals, and staged_shortlist_kernel builds the shortlist from the two lists -- instead of the
second merge, the combine over all candidates and the shortlist pass over all candidates.

Every case runs the same pair, candidates and workspace with HBX_STAGED=2 and HBX_STAGED_TAIL=0 (the earlier launch
sequence) and unset (the short tail).  Both tails run the same scoring launches with the same splits and take every
interval with the same functions from the same operands, so every record field -- `shortlist` included -- and
hbx_kde_acquire_stats must be equal.  Pairs are fitted by tests/test_gpu_staged.py's recipe (BOHB's split,
normal-reference bandwidths, categorical ones capped at 0.8), both KDEs on the coarse 32x32 instance.
"""
import struct

import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

CAP = 4096  # STAGED_LIST_CAP: seeds at most, and listed candidates at most of a split list launch
OVERFLOW = 1  # HBX_ACQ_OVERFLOW


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


def _run(pair, Cd, ws, monkeypatch, tail, **kw):
    if tail:
        monkeypatch.delenv("HBX_STAGED_TAIL", raising=False)
    else:
        monkeypatch.setenv("HBX_STAGED_TAIL", "0")
    rec = pair.acquire(Cd, workspace=ws, **kw)
    st = pair.acquire_stats(ws, len(Cd))
    assert st["staged"], st
    return rec, st


def _ab(pair, C, monkeypatch, device, **kw):
    """(record, stats) of the short tail, equal to the earlier launch sequence's on the same workspace -- run
    before it and after it, so either tail also starts from the state the other one left."""
    import torch
    monkeypatch.setenv("HBX_STAGED", "2")
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    new0, st_new0 = _run(pair, Cd, ws, monkeypatch, True, **kw)
    old, st_old = _run(pair, Cd, ws, monkeypatch, False, **kw)
    new, st_new = _run(pair, Cd, ws, monkeypatch, True, **kw)
    print("tail off", old, st_old, "tail on", new, st_new)
    assert _record(new) == _record(old), (new, old)
    assert _record(new0) == _record(old), (new0, old)
    assert st_new == st_old and st_new0 == st_old, (st_new0, st_old, st_new)
    return new, st_new


@pytest.fixture(scope="module")
def bench_like(device):
    """test_gpu_staged.py's: 24c + 8u with 4 levels, 400 observations, 4099 candidates."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=211)
    pair = _fit(X, S.make_losses(400, seed=212), vt, device)
    C = S.make_candidates(4099, 24, 8, 4, seed=213)
    return pair, vt, C


@pytest.mark.parametrize("nc", [1, 33, 513, 1025, 4097])
def test_sizes(device, monkeypatch, bench_like, nc):
    """Candidate counts one past a wave tile, a 512-candidate block, a selection block and the list capacity, and
    a single candidate: most candidates pruned, a few tens evaluated."""
    pair, vt, C = bench_like
    new, st = _ab(pair, C[:nc], monkeypatch, device)
    assert 0 <= new.index < nc
    assert 1 <= st["evaluated"] <= nc


def test_stage_one_splits_its_observations(device, monkeypatch):
    """900 observations (765 bad: 12 chunks) and 700 candidates: few tiles and at least 8 chunks, so stage 1 and
    the list launches split their observations in two or more -- staged_l_kernel merges l, the tail kernel the
    survivors' partials."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(900, 24, 8, 4, seed=311)
    pair = _fit(X, S.make_losses(900, seed=312), vt, device)
    assert pair.nmax >= 8 * 64
    C = S.make_candidates(700, 24, 8, 4, seed=313)
    new, st = _ab(pair, C, monkeypatch, device)
    assert new.index >= 0 and st["evaluated"] >= 1


def test_seed_list_overflows(device, monkeypatch, bench_like):
    """test_tie_overflowing_the_seed_cap's candidates: 5000 copies of one row behind 1000 others fill the seed list,
    the rest arrive as survivors, and every copy is shortlisted."""
    pair, vt, C = bench_like
    monkeypatch.setenv("HBX_STAGED", "0")
    best = pair.acquire(C[:1000]).index  # (the pick of the first 1000, as that test takes it from the oracle)
    assert best >= 0
    C2 = np.vstack([C[:1000], np.repeat(C[best:best + 1], 5000, axis=0)])
    new, st = _ab(pair, C2, monkeypatch, device)
    assert new.index == best
    assert st["seeds"] == CAP and st["survivors"] >= 5001 - CAP, st
    assert new.shortlist >= 5001 and new.near >= 5001


def test_unsplit_survivor_launch(device, monkeypatch):
    """test_nothing_pruned's pair (8 continuous dims, pdfs far above 1e-8) with 6000 candidates: every candidate
    survives, more than the list capacity, so the survivor launch runs unsplit and scatters its own estimates --
    the tail kernel takes their intervals from a.eg."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(8, 0)
    X = S.make_observations(300, 8, 0, 1, seed=221)
    pair = _fit(X, S.make_losses(300, seed=222), vt, device)
    C = S.make_candidates(6000, 8, 0, 1, seed=223)
    new, st = _ab(pair, C, monkeypatch, device)
    assert st["seeds"] + st["survivors"] == len(C) and st["survivors"] > CAP, st
    assert new.index >= 0


def test_every_score_exactly_one(device, monkeypatch):
    """test_every_score_exactly_one's candidates: every evaluated candidate is a certain tie, so the shortlist is
    first1 alone."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=231)
    pair = _fit(X, S.make_losses(400, seed=232), vt, device)
    C = S.make_candidates(700, 24, 8, 4, seed=233)
    C[:, :24] += 4.0
    new, st = _ab(pair, C, monkeypatch, device)
    assert (new.index, new.score) == (0, 1.0)
    assert st["seeds"] + st["survivors"] == len(C)
    assert new.shortlist == 1


def test_nan_l_in_some_rows(device, monkeypatch):
    """test_nan_l_single_level_dim's pair: l is NaN for every candidate off the good KDE's single level."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=241)
    losses = S.make_losses(400, seed=242)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 24] = 2.0
    pair = _fit(X, losses, vt, device)
    assert pair.good.nlev[24] == 1
    C = S.make_candidates(2050, 24, 8, 4, seed=243)
    new, st = _ab(pair, C, monkeypatch, device)
    assert new.index >= 0 and C[new.index, 24] == 2.0
    assert st["seeds"] + st["survivors"] <= int((C[:, 24] == 2.0).sum())


def test_nan_l_in_all_rows(device, monkeypatch):
    """test_nan_l_everywhere's pair: nothing seeded, nothing survives, an empty shortlist, index -1."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=251)
    losses = S.make_losses(400, seed=252)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 5] = 0.25
    pair = _fit(X, losses, vt, device)
    assert pair.good.bw[5] == 0
    C = S.make_candidates(1500, 24, 8, 4, seed=253)
    new, st = _ab(pair, C, monkeypatch, device)
    assert (new.index, new.shortlist) == (-1, 0)
    assert (st["seeds"], st["survivors"], st["evaluated"]) == (0, 0, 0), st


def _narrow(bw):
    bw = bw.copy()
    bw[0] = 0.004
    return bw


@pytest.mark.parametrize("which", ["bad", "good"])
def test_rescue_markers(device, monkeypatch, which):
    """test_rescue_markers_among_the_seeds' construction (one KDE narrow in dim 0, every candidate at x_0 = 1.6):
    against the bad KDE every g estimate the staged path computes is a rescue marker, which the tail kernel
    re-scores in place of the combine; against the good KDE every l estimate is one, which staged_l_kernel
    re-scores before either tail."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=261)
    kw = {"bw_bad": _narrow} if which == "bad" else {"bw_good": _narrow}
    pair = _fit(X, S.make_losses(400, seed=262), vt, device, **kw)
    C = S.make_candidates(1300, 24, 8, 4, seed=263)
    C[:, 0] = 1.6
    new, st = _ab(pair, C, monkeypatch, device)
    assert st["seeds"] >= 1
    if which == "bad":
        assert st["seeds"] + st["survivors"] == len(C), st  # no marked seed lowers U_seed


def test_overflow_from_l(device, monkeypatch):
    """16 continuous dims whose good bandwidths are 2e-20 over observations within 1e-19 of the origin: at an
    observation row ln l is about 16 (45.4 - 0.92) - ln 60 = 707, past the overflow flag's 700, while the bad KDE
    (bandwidths 1e-10, ln g at most 16 (23.0 - 0.92) = 354) stays far below the staged path's guard.  Half of the
    300 candidates are good rows; the others lie 1e-18 away, where l underflows and the l-only bound prunes them.
    Both tails must set HBX_ACQ_OVERFLOW and shortlist every candidate."""
    rs = np.random.RandomState(331)
    n, D, nc = 400, 16, 300
    X = 1e-19 * rs.rand(n, D)
    losses = rs.rand(n)
    vt = "c" * D
    pair = _fit(X, losses, vt, device, bw_good=lambda bw: np.full(D, 2e-20), bw_bad=lambda bw: np.full(D, 1e-10))
    g_idx, _ = O.bohb_split(X, losses, D + 1)
    C = np.vstack([X[g_idx][rs.randint(0, len(g_idx), size=nc // 2)],
                   1e-18 + 1e-19 * rs.rand(nc - nc // 2, D)])
    new, st = _ab(pair, C[rs.permutation(nc)], monkeypatch, device)
    assert new.flags & OVERFLOW, new
    assert new.shortlist == nc
    assert st["evaluated"] < nc, st  # some candidates were pruned: their flag and bound come from the survivor pass


def test_index_base_without_sync(device, monkeypatch, bench_like):
    """index_base = 3 * 2^33 with sync=False: the record stays on the device (fetch_bytes) and equals the earlier
    sequence's."""
    import torch
    from hpbandster_amd import kde
    pair, vt, C = bench_like
    C = C[:2000]
    base = 3 * 2 ** 33
    new, st = _ab(pair, C, monkeypatch, device, index_base=base)
    assert new.index >= base
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    recs = []
    for tail in (False, True):
        if tail:
            monkeypatch.delenv("HBX_STAGED_TAIL", raising=False)
        else:
            monkeypatch.setenv("HBX_STAGED_TAIL", "0")
        rv = pair.acquire(Cd, index_base=base, workspace=ws, sync=False)
        recs.append(kde.AcqResult.from_bytes(kde.fetch_bytes(rv)))
        assert pair.acquire_stats(ws, len(C)) == st
    assert _record(recs[0]) == _record(recs[1]) == _record(new)


def test_two_calls_on_one_workspace(device, monkeypatch, bench_like):
    """Two short-tail calls back to back on one workspace, 4099 candidates and then 1300 others: the second record
    and its stats equal those of a fresh workspace (the preliminary list's length, the shortlist count and the
    marker count start clean)."""
    import torch
    pair, vt, C = bench_like
    monkeypatch.setenv("HBX_STAGED", "2")
    monkeypatch.delenv("HBX_STAGED_TAIL", raising=False)
    C1, C2 = C, np.ascontiguousarray(C[2500:3800][::-1])
    d1, d2 = torch.from_numpy(C1).to(device), torch.from_numpy(C2).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C1)), dtype=torch.uint8, device=device)
    first = pair.acquire(d1, workspace=ws)
    assert pair.acquire_stats(ws, len(C1))["staged"]
    second = pair.acquire(d2, workspace=ws)
    st2 = pair.acquire_stats(ws, len(C2))
    fresh_ws = torch.empty(pair.workspace_bytes(len(C2)), dtype=torch.uint8, device=device)
    fresh = pair.acquire(d2, workspace=fresh_ws)
    assert _record(second) == _record(fresh), (second, fresh)
    assert st2 == pair.acquire_stats(fresh_ws, len(C2)) and st2["staged"]
    assert first.index >= 0 and 0 <= second.index < len(C2)
