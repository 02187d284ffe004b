"""Staged single acquisitions with chosen seed-list lengths (hbx_staged.hip): the seed kernel's reduction of the block
maxima with 16-byte loads, the seeds' merge with every partial loaded before the marker test, the overflow guard
from KdeParams; and, in a case of its own with nothing pruned, the tail kernel's merge of the survivors' partials.

2000 observations (300 good: five chunks; 1700 bad: the list launches split their observations in six) and 66 000
candidates (258 one-tile blocks: stage 1 runs unsplit, so its epilogue leaves lhi and the seed kernel reduces 258
maxima, 64 float4 and two floats behind them).  k candidates are copies of one good observation, where l is
largest (its own kernel term); the others are random points moved by 3 in the first dim, so far below in l that
neither ln 4 nor the coarse estimates' bounds reach them: exactly the k copies are seeded.  Every record field and
hbx_kde_acquire_stats must equal those of HBX_STAGED_TAIL=0 (the merge kernel in place of the tail kernel's merge)
and of HBX_STAGE1_LHI=0 (Lmax from staged_l_kernel's atomic, not the reduction) on the same workspace, and the Lmax
word must be equal with the fold on and off.
"""
import struct

import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

NC = 66000
COUNTS = [1, 31, 32, 33, 61, 64, 65, 257]


def _record(r):
    """Every field of a record, NaN-safe."""
    return (r.index, struct.pack("<ddd", r.score, r.pdf_l, r.pdf_g), r.flags, r.near, struct.pack("<f", r.rel),
            r.shortlist)


@pytest.fixture(scope="module")
def setup(device):
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(2000, 24, 8, 4, seed=811)
    g_idx, b_idx = O.bohb_split(X, S.make_losses(2000, seed=812), 33)
    cat = np.array([v == "u" for v in vt])
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    bwg[cat] = np.minimum(bwg[cat], 0.8)
    bwb[cat] = np.minimum(bwb[cat], 0.8)
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt), device=device)
    assert (pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1  # both on the coarse 32x32 instance
    assert pair.nmax == 1700
    C = S.make_candidates(NC, 24, 8, 4, seed=813)
    C[:, 0] += 3.0  # two or more away from every observation in dim 0: about 30 in ln l at the bandwidth of 0.26
    ws = torch.empty(pair.workspace_bytes(NC), dtype=torch.uint8, device=device)
    return pair, C, np.asarray(pair.good.data)[0].copy(), ws


def _run(pair, Cd, ws, monkeypatch, tail=True, fold=True):
    for name, on in (("HBX_STAGED_TAIL", tail), ("HBX_STAGE1_LHI", fold)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "0")
    rec = pair.acquire(Cd, workspace=ws)
    st = pair.acquire_stats(ws, len(Cd))
    s1 = pair.acquire_stage1(ws, len(Cd))
    assert st["staged"] and s1["lhi_epilogue"] == fold, (st, s1)
    return rec, st, s1["lmax_bits"]


@pytest.mark.parametrize("k", COUNTS)
def test_seed_list_lengths(device, monkeypatch, setup, k):
    import torch
    pair, C, row, ws = setup
    C = C.copy()
    pos = np.unique(np.linspace(3, NC - 2, k).astype(int))  # the first block, the last one, and between
    assert len(pos) == k
    C[pos] = row
    monkeypatch.setenv("HBX_STAGED", "2")
    Cd = torch.from_numpy(C).to(device)
    new0, st0, lm0 = _run(pair, Cd, ws, monkeypatch)
    old_tail, st_tail, lm_tail = _run(pair, Cd, ws, monkeypatch, tail=False)
    old_fold, st_fold, lm_fold = _run(pair, Cd, ws, monkeypatch, fold=False)
    new, st, lm = _run(pair, Cd, ws, monkeypatch)
    assert st["seeds"] == k, st  # the premise: the copies and nothing else
    assert 0 <= new.index < NC, new
    assert _record(new) == _record(new0) == _record(old_tail) == _record(old_fold), (new, new0, old_tail, old_fold)
    assert st == st0 == st_tail == st_fold, (st, st0, st_tail, st_fold)
    assert lm == lm0 == lm_tail == lm_fold, (hex(lm), hex(lm0), hex(lm_tail), hex(lm_fold))


def test_survivors_partials_merged_by_the_tail(device, monkeypatch):
    """8 continuous dims, 2000 observations (1700 bad: the list launches split in six), 3000 candidates, every pdf
    far above 1e-8: nothing is pruned, every candidate is a seed or a survivor, and the survivors -- fewer than the
    list capacity -- leave split partials that the tail kernel merges (the merge kernel under HBX_STAGED_TAIL=0).
    Both records equal each other in every field, the pick is the C oracle's, and pdf_l, pdf_g its bits."""
    import torch
    from oracle import c_oracle
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(8, 0)
    X = S.make_observations(2000, 8, 0, 1, seed=821)
    g_idx, b_idx = O.bohb_split(X, S.make_losses(2000, seed=822), 9)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt), device=device)
    assert (pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1 and pair.nmax == 1700
    C = S.make_candidates(3000, 8, 0, 1, seed=823)
    Cd = torch.from_numpy(C).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "2")
    out = []
    for tail in (True, False, True):
        if tail:
            monkeypatch.delenv("HBX_STAGED_TAIL", raising=False)
        else:
            monkeypatch.setenv("HBX_STAGED_TAIL", "0")
        rec = pair.acquire(Cd, workspace=ws)
        out.append((_record(rec), pair.acquire_stats(ws, len(C))))
    st = out[0][1]
    assert st["staged"] and st["survivors"] > 0 and st["seeds"] + st["survivors"] == len(C), st  # the premise
    assert st["survivors"] <= 4096  # within the split launch's capacity: partials, not a scatter
    assert out[0] == out[1] == out[2], out
    l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
    g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    want = O.select(l, g)[0]
    assert rec.index == want and (rec.pdf_l, rec.pdf_g) == (l[want], g[want]), (rec, want)
