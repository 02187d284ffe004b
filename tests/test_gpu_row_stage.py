"""Row staging of the coarse 32x32 scoring instances (hbx_score_h32.hip): a block's candidate rows reach the
operand build through LDS, copied coalesced one column tile at a time, instead of every lane reading its own row
from global memory.  Only where the doubles are read from changes, so every estimate -- and with it every field of
an acquisition's record, the staged path's counts included -- is bit for bit what the direct path gives.

Every case runs the same pair, candidates and workspace twice, with HBX_ROW_STAGE=0 (the direct path) and with the
switch unset, compares the two records field by field, and checks the pick against the C oracle.  Pairs are built
as in test_gpu_staged.py (categorical bandwidths capped at 0.8: unsigned KDEs, the coarse instance), 52 good and
297 bad observations.
"""
import struct

import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_staged import _bits, _fit, _oracle_pick

pytestmark = pytest.mark.gpu

N_OBS = 350  # BOHB's split: 52 good, 297 bad rows


def _pair(dc, du, levels, seed, device):
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(dc, du)
    X = S.make_observations(N_OBS, dc, du, levels, seed=seed)
    return _fit(X, S.make_losses(N_OBS, seed=seed + 1), vt, device), vt


def _coarse(pair):
    return bool((pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1)


def _equal(on, off):
    assert on.index == off.index, (on.index, off.index)
    for f in ("score", "pdf_l", "pdf_g"):
        assert _bits(getattr(on, f)) == _bits(getattr(off, f)), (f, getattr(on, f), getattr(off, f))
    assert (on.flags, on.shortlist, on.near) == (off.flags, off.shortlist, off.near)
    assert struct.pack("<f", on.rel) == struct.pack("<f", off.rel), (on.rel, off.rel)


def _twice(pair, C, monkeypatch, device, **kw):
    """(record with the rows staged, its stats) after checking both against the direct path's."""
    import torch
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    nc = len(C)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_ROW_STAGE", "0")
    off = pair.acquire(Cd, workspace=ws, **kw)
    st_off = pair.acquire_stats(ws, nc)
    monkeypatch.delenv("HBX_ROW_STAGE")
    on = pair.acquire(Cd, workspace=ws, **kw)
    st_on = pair.acquire_stats(ws, nc)
    _equal(on, off)
    assert st_on == st_off, (st_on, st_off)
    return on, st_on


@pytest.fixture(scope="module")
def wide(device):
    """24c + 8u with 4 levels (D = 32: a row fills the stride-33 slice, two column tiles do not fit the ring), 4097
    candidates and the oracle's pdfs; a prefix's oracle pick comes from the same pdfs."""
    from hpbandster_amd import synthetic as S
    pair, vt = _pair(24, 8, 4, 311, device)
    assert _coarse(pair)
    C = S.make_candidates(4097, 24, 8, 4, seed=313)
    _, l, g = _oracle_pick(pair, vt, C)
    return pair, vt, C, l, g


@pytest.mark.parametrize("nc", [1, 31, 33, 64, 65, 511, 513, 1025])
def test_ragged_edges(device, monkeypatch, wide, nc):
    """A wave with fewer than 32 rows and an empty second column tile (1, 31; 65: the second wave's), a second
    tile of one row (33), a block whose later waves have no rows (64), a last wave of 63 rows (511), one row past
    a block (513, 1025)."""
    pair, vt, C, l, g = wide
    on, _ = _twice(pair, C[:nc], monkeypatch, device)
    assert on.index == O.select(l[:nc], g[:nc])[0]


@pytest.mark.parametrize("dc,du,levels,coarse", [(8, 0, 1, True), (3, 2, 4, False), (8, 2, 4, True),
                                                 (16, 0, 1, True), (16, 4, 4, True), (30, 10, 2, True)])
def test_other_widths(device, monkeypatch, dc, du, levels, coarse):
    """1025 candidates at other row widths.  16c + 0u and 16c + 4u: the narrowest staged rows (D = 16, 20: four
    and three rows per 64-lane pass of the copy, the latter with idle lanes), without and with a one-hot step.  8c + 0u and 8c + 2u:
    rows below one cache line are read in place under both settings.  3c + 2u lies below the 32x32 buckets (they
    start at 8 continuous dims), so no coarse instance runs and the switch must change nothing.  30c + 10u with
    2 levels: D = 40 is wider than the slice, both settings read the rows in place."""
    from hpbandster_amd import synthetic as S
    pair, vt = _pair(dc, du, levels, 321 + dc, device)
    assert _coarse(pair) == coarse
    C = S.make_candidates(1025, dc, du, levels, seed=323 + dc)
    on, _ = _twice(pair, C, monkeypatch, device)
    assert on.index == _oracle_pick(pair, vt, C)[0]


@pytest.mark.parametrize("env,val", [("HBX_PAIR1", "0"), ("HBX_PAIR1", "1"), ("HBX_SCORE_PAIR", "0")])
def test_kernel_choice(device, monkeypatch, wide, env, val):
    """2049 candidates: the pair kernel (two column tiles per wave), the one-tile pair kernel, and with
    HBX_SCORE_PAIR=0 the one-KDE kernel, twice."""
    pair, vt, C, l, g = wide
    monkeypatch.setenv(env, val)
    on, _ = _twice(pair, C[:2049], monkeypatch, device)
    assert on.index == O.select(l[:2049], g[:2049])[0]


def test_staged_list_gathered(device, monkeypatch, wide):
    """HBX_STAGED=2 at 4097 candidates with an index base: the seeds' list launch gathers non-adjacent rows into the
    slice and writes split partials; seeds, survivors and evaluated counts may not move."""
    pair, vt, C, l, g = wide
    monkeypatch.setenv("HBX_STAGED", "2")
    base = 5 * 2 ** 32
    on, st = _twice(pair, C, monkeypatch, device, index_base=base)
    assert st["staged"] and st["seeds"] >= 2, st
    assert on.index == O.select(l, g)[0] + base


def test_staged_nothing_pruned(device, monkeypatch):
    """8 continuous dims, every pdf far above 1e-8 (test_gpu_staged.py test_nothing_pruned): every candidate is a
    seed or a survivor (1537 of them: both lists within the split launch's 4096; D = 8 rows are read in place)."""
    from hpbandster_amd import synthetic as S
    pair, vt = _pair(8, 0, 1, 331, device)
    assert _coarse(pair)
    C = S.make_candidates(1537, 8, 0, 1, seed=333)
    monkeypatch.setenv("HBX_STAGED", "2")
    on, st = _twice(pair, C, monkeypatch, device)
    assert st["staged"] and st["seeds"] + st["survivors"] == len(C) and st["survivors"] > 0, st
    assert on.index == _oracle_pick(pair, vt, C)[0]


def test_staged_survivors_unsplit(device, monkeypatch):
    """16 continuous dims, 8300 candidates within a twentieth of a good observation: every l is far above 1e-8 and
    nothing is pruned.  The seed list takes 4096 of them; the others, more than the split launch's 4096, make the
    list instance run unsplit, one block per tile of the list, gathering staged rows and scattering its own
    estimates."""
    from hpbandster_amd import synthetic as S
    pair, vt = _pair(16, 0, 1, 341, device)
    assert _coarse(pair)
    rs = np.random.RandomState(343)
    C = pair.good.data[rs.randint(0, len(pair.good.data), size=8300)] + 0.05 * rs.randn(8300, 16)
    monkeypatch.setenv("HBX_STAGED", "2")
    on, st = _twice(pair, C, monkeypatch, device)
    assert st["staged"] and st["survivors"] > 4096, st
    assert on.index == _oracle_pick(pair, vt, C)[0]


def test_topk(device, monkeypatch, wide):
    """acquire_topk, k = 64 of 2049: every entry equal."""
    pair, vt, C, l, g = wide
    monkeypatch.setenv("HBX_ROW_STAGE", "0")
    off = pair.acquire_topk(C[:2049], 64)
    monkeypatch.delenv("HBX_ROW_STAGE")
    on = pair.acquire_topk(C[:2049], 64)
    assert on.count == off.count == 64 and (on.shortlist, on.flags) == (off.shortlist, off.flags)
    for f in ("index", "score", "pdf_l", "pdf_g", "rel"):
        assert getattr(on, f).tobytes() == getattr(off, f).tobytes(), f
    assert on.index[0] == O.select(l[:2049], g[:2049])[0]


def test_non_finite_rows(device, monkeypatch, wide):
    """A row holding NaN in a continuous column, one holding NaN in a categorical column and one with a level no
    observation has (7 of 4 levels), in the first and the second column tile of a wave."""
    pair, vt, C, l, g = wide
    C = C[:700].copy()
    C[5, 3] = np.nan
    C[40, 27] = np.nan
    C[41, 30] = 7.0
    C[130, 0] = np.nan
    on, _ = _twice(pair, C, monkeypatch, device)
    assert on.index == _oracle_pick(pair, vt, C)[0]
    assert on.index not in (5, 40, 130)
