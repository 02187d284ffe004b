"""Operand build from staged rows against the direct build (HBX_ROW_STAGE=0), byte for byte, under permuted column
orders (tests/dim_orders.py): the coarse 32x32 instances copy a block's candidate rows through LDS one column tile at
a time and build their B operands from there; with the switch off every lane reads its own row in global memory.
Only where the doubles come from differs, so every record field and the staged path's counts must be equal.

Row widths 16 (12c + 4u), 24 (18c + 6u), 32 (24c + 8u) and 33 (25c + 8u: the widest staged stride), each built
c-first and permuted (categorical first, alternating, lone ends, a random order), so continuous and one-hot slots
read columns all over the row ("straddle", the fifth order of that file, needs more than 65 dims: wider than any
staged row, read in place under both settings).  Candidate counts 1, 31, 33, 63, 65, 511, 513: partly filled
tiles, waves and blocks.  Kernels: the two-tile pair kernel (HBX_PAIR1=0), the one-tile pair kernel (HBX_PAIR1=1), and with HBX_STAGED=2 the
list kernel behind stage 1.
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests import dim_orders as DO
from tests.test_gpu_row_stage import _coarse, _twice

pytestmark = pytest.mark.gpu

WIDTHS = {16: (12, 4), 24: (18, 6), 32: (24, 8), 33: (25, 8)}
ORDERS = ["cat_first", "alternate", "lone_ends", "random7"]
NCS = [1, 31, 33, 63, 65, 511, 513]
KERNELS = {"pair": {"HBX_STAGED": "0", "HBX_PAIR1": "0"}, "pair1": {"HBX_STAGED": "0", "HBX_PAIR1": "1"},
           "list": {"HBX_STAGED": "2"}}
N_OBS = 350


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D", sorted(WIDTHS))
def test_staged_build_equals_direct(device, monkeypatch, D, order):
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dc, du = WIDTHS[D]
    perm = DO.order_perm(order, dc, du)
    vt0 = DO.cfirst_vt(dc, du)
    X0 = S.make_observations(N_OBS, dc, du, 4, seed=900 + D)
    g_idx, b_idx = O.bohb_split(X0, S.make_losses(N_OBS, seed=901 + D), D + 1)
    cat = np.array([v == "u" for v in vt0])
    with np.errstate(all="ignore"):
        bwg0, bwb0 = O.normal_reference_bw(X0[g_idx]), O.normal_reference_bw(X0[b_idx])
    bwg0[cat], bwb0[cat] = np.minimum(bwg0[cat], 0.8), np.minimum(bwb0[cat], 0.8)
    nlg0, nlb0 = O.num_levels(X0[g_idx], vt0), O.num_levels(X0[b_idx], vt0)
    p = DO.permute(perm, X=X0, C=S.make_candidates(max(NCS), dc, du, 4, seed=902 + D), vt=vt0)
    pair = kde.fit_pair_from_rows(p["X"], g_idx, b_idx, p["vt"], DO.permute(perm, bw=bwg0)["bw"],
                                  DO.permute(perm, bw=bwb0)["bw"], DO.permute(perm, nlev=nlg0)["nlev"],
                                  DO.permute(perm, nlev=nlb0)["nlev"], device=device)
    assert _coarse(pair)
    for name, env in KERNELS.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for nc in NCS:
            on, st = _twice(pair, p["C"][:nc], monkeypatch, device)
            assert st["staged"] == (name == "list"), (name, nc, st)
            assert 0 <= on.index < nc
        for k in env:
            monkeypatch.delenv(k)
