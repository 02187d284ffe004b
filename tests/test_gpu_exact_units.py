"""The acquisition's exact re-score with a unit's (observation, dim) factors spread over lanes (hbx_exact.hip,
exact_unit_spread in hbx_exact_impl.h): four adjacent lanes per observation evaluate every fourth dim's factor and
multiply them in dim order, the unit sums in numpy's pairwise order as before.  The record's pdf_l and pdf_g must be
the C oracle's reference arithmetic bit for bit.  That kernel runs behind the staged acquisition's short tail, so
every call is made with HBX_STAGED=2 and acquire_stats must report `staged` for D = 32 and D = 33, whose KDEs are on
the coarse 32x32 instance.  D = 1 (below the 32x32 buckets) and D = 65 (57 continuous dims: past them) cannot stage:
there the one-observation-per-thread kernel is what is checked.

Observation counts per KDE: 1; 262, 263, 264 (263 is the longest unit of the depth-5 split tree, one past a 256-
observation pass: 264 splits differently again); 8192 (one full ufunc buffer: 32 units of 256) and 8193 (a second
buffer of one observation).  Dims: 1; 32 (24c + 8u, the bench's: four full chunks of eight dims); 33 (25c + 8u,
beyond the issue's set: a last chunk with one dim in range, three lanes of a group without a factor); 65 (57c + 8u).  Each pair scores three candidates near observations, one call each (the winner is the candidate, so the
record shows its two pdfs) and one call of 1100 candidates, checked at the winner.
"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 262, 263, 264, 8192, 8193]
DIMS = {1: (1, 0), 32: (24, 8), 33: (25, 8), 65: (57, 8)}
LEVELS = 4


def _bits(x):
    return "nan" if x != x else struct.pack("<d", x)


def _pair(n, D, device):
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    from oracle import kde_oracle as O
    dc, du = DIMS[D]
    vt = S.var_type_string(dc, du)
    X = S.make_observations(2 * n, dc, du, LEVELS, seed=1000 + 7 * n + D)
    if n == 1:
        X[:, dc:] = X[0, dc:]  # one observation per KDE: its level is the only one either KDE has seen
    g_idx, b_idx = np.arange(n), np.arange(n, 2 * n)
    nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)

    def bw(nlev):
        h = np.full(D, 0.25)
        h[dc:] = np.where(np.asarray(nlev)[dc:] > 1, 0.4, 0.0)
        return h
    pair = kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bw(nlg), bw(nlb), nlg, nlb, device=device)
    rs = np.random.RandomState(2000 + n + D)
    C = np.vstack([X[0], X[n], X[n - 1]])
    C[:, :dc] += 0.05 * rs.randn(3, dc)
    return pair, vt, C, rs


def _oracle(pair, vt, C):
    from oracle import c_oracle
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    return l, g


@pytest.mark.parametrize("D", sorted(DIMS))
@pytest.mark.parametrize("n", NS)
def test_pdfs_are_the_oracles(device, monkeypatch, n, D):
    import torch
    monkeypatch.setenv("HBX_STAGED", "2")
    monkeypatch.delenv("HBX_STAGED_TAIL", raising=False)
    from hpbandster_amd import synthetic as S
    pair, vt, C, rs = _pair(n, D, device)
    l, g = _oracle(pair, vt, C)
    coarse = bool((pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1)
    assert coarse == (D in (32, 33)), (D, n)  # these stage: the wide kernel is what runs there

    def acquire(Cd):
        ws = torch.empty(pair.workspace_bytes(len(Cd)), dtype=torch.uint8, device=device)
        r = pair.acquire(Cd, workspace=ws)
        assert pair.acquire_stats(ws, len(Cd))["staged"] == coarse
        return r
    assert np.all(l > 0) and np.all(g > 0), (l, g)  # the premise: pdfs with bits to compare
    for i in range(len(C)):
        r = acquire(torch.from_numpy(np.ascontiguousarray(C[i:i + 1])).to(device))
        assert r.index == 0, r
        assert (_bits(r.pdf_l), _bits(r.pdf_g)) == (_bits(l[i]), _bits(g[i])), (r, l[i], g[i])
    dc, du = DIMS[D]
    big = np.vstack([S.make_candidates(1097, dc, du, LEVELS, seed=3000 + n + D), C])
    if n == 1:
        big[:, dc:] = C[0, dc:]
    r = acquire(torch.from_numpy(big).to(device))
    assert 0 <= r.index < len(big), r
    lw, gw = _oracle(pair, vt, big[r.index:r.index + 1])
    assert (_bits(r.pdf_l), _bits(r.pdf_g)) == (_bits(lw[0]), _bits(gw[0])), (r, lw[0], gw[0])
