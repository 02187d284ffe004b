"""Grouped acquisition with S get_config requests per bracket (hbx_kde_acquire_groups_batch,
GroupModel.acquire_requests) on the GPU: record (b, s) equals the C oracle's pick over cand[b][s]
(c_oracle.kde_pdf(exact=True) + kde_oracle.select) and record b of the one-request call over that pool, bit for bit:
index, score and both pdfs.  The groups are tests/test_gpu_groups.py's.
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import NEAR_TIE, NO_MODEL, OVERFLOW, UNSUPPORTED, _groups, _oracle, _same

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (0, 3), (5, 2), (24, 8)]
# S * C candidates per group flatten to 64-candidate tiles; the tile screen runs from 3 tiles on (hbx_groups.hip):
# (3, 1) a pool under one tile and (3, 40) two tiles that straddle requests, the second partial -- the
# chunk-splitting screen over the flattened pool; (4, 37) and (9, 20) three tiles that straddle requests, the last
# one partial and one wave of the block without a tile; (5, 64) five tiles, more than a block's four waves (a
# second block with one live wave); (12, 64) twelve tiles, three full blocks per group -- the tile screen
REQUESTS = [(3, 1), (3, 40), (4, 37), (5, 64), (9, 20), (12, 64)]


def _check(device, dc, du, S, C):
    """every record of one batched call against the oracle, the one-request call and the per-kind facts"""
    from hpbandster_amd import groups
    X, losses, seg, vt, levels, pool, kinds = _groups(dc, du, S * C)
    B, D = len(seg) - 1, dc + du
    cands = np.ascontiguousarray(pool.reshape(B, S, C, D))
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    dup = {}
    if C > 1:  # the duplicate: the oracle's winner of every request of group 5 copied to a neighbouring index
        for s in range(S):
            l, g = _oracle(gm, X, seg, vt, cands[:, s], 5)
            w, _ = O.select(l, g)
            assert w >= 0
            j = w + 1 if w + 1 < C else w - 1
            cands[5, s, j] = cands[5, s, w]
            dup[s] = min(w, j)
    picks = gm.acquire_requests(cands)
    assert len(picks) == B and picks.index.shape == (B, S)
    for s in range(S):
        one = gm.acquire(np.ascontiguousarray(cands[:, s]))
        for b in range(B):
            kind = kinds.get(b)
            where = (b, s, kind)
            rec = (picks.index[b, s], picks.score[b, s], picks.pdf_l[b, s], picks.pdf_g[b, s])
            if kind == "no_model" or kind == "unsupported":
                assert picks.flags[b, s] & (NO_MODEL if kind == "no_model" else UNSUPPORTED), where
                assert rec[0] == -1 and all(np.isnan(v) for v in rec[1:]), where
                assert picks.shortlist[b, s] == 0 and picks.near[b, s] == 0, where
                continue
            assert not picks.flags[b, s] & (NO_MODEL | UNSUPPORTED), where
            l, g = _oracle(gm, X, seg, vt, cands[:, s], b)
            want, scores = O.select(l, g)
            assert rec[0] == want, (where, rec, want, picks.flags[b, s])
            if want >= 0:
                assert _same(rec[2], l[want]) and _same(rec[3], g[want]) and rec[1] == scores[want], where
            else:
                assert all(np.isnan(v) for v in rec[1:]), where
            assert rec[0] == one.index[b] and _same(rec[1], one.score[b]) and _same(rec[2], one.pdf_l[b]) and \
                _same(rec[3], one.pdf_g[b]), (where, rec)
            if kind == "const_cont":
                assert want == -1 and np.all(np.isnan(l)) and np.all(np.isnan(g))
            if kind == "one_level":
                assert picks.flags[b, s] & OVERFLOW and picks.shortlist[b, s] == C  # exact-only: all re-scored
            if kind == "all_far":
                assert want == 0 and rec[1] == 1.0 and np.all(scores == 1.0)
                if C > 1:
                    assert picks.flags[b, s] & NEAR_TIE
            if kind == "dup" and C > 1:
                assert picks.flags[b, s] & NEAR_TIE and picks.near[b, s] >= 2
                assert rec[0] == dup[s]


@pytest.mark.parametrize("S,C", REQUESTS)
@pytest.mark.parametrize("dc,du", SHAPES)
def test_every_record_equals_oracle_and_one_request_call(device, dc, du, S, C):
    _check(device, dc, du, S, C)


@pytest.mark.parametrize("screen,S,C", [("1", 12, 64), ("1", 4, 37), ("2", 3, 40), ("2", 3, 1)])
def test_the_other_screen_forced(device, monkeypatch, screen, S, C):
    """HBX_GROUPS_SCREEN = 1: the chunk-splitting screen over pools the rule gives to the tile screen; 2: the tile
    screen over pools below the rule's threshold (two and three of a block's four waves without a tile)."""
    monkeypatch.setenv("HBX_GROUPS_SCREEN", screen)
    _check(device, 24, 8, S, C)


def test_requests_do_not_see_one_another(device):
    """Request 0: every candidate far (every score exactly 1, index 0); request 1: observation rows plus noise
    (scores far below 1); request 2: request 1 with its winner duplicated at a later index.  A bound or a
    first-certain-1 taken over the group's whole pool loses request 0's pick or request 2's tie."""
    from hpbandster_amd import groups
    from hpbandster_amd import synthetic as S_
    dc, du, n, C = 6, 0, 200, 64
    rs = np.random.RandomState(7)
    X = S_.make_observations(n, dc, du, 3, seed=31)
    losses = S_.make_losses(n, seed=32)
    seg = np.array([0, n], dtype=np.int64)
    vt = S_.var_type_string(dc, du)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    cands = np.empty((1, 3, C, dc))
    cands[0, 0] = 5.0 + rs.rand(C, dc)
    cands[0, 1] = X[rs.randint(0, n, size=C)] + 0.01 * rs.randn(C, dc)
    l, g = _oracle(gm, X, seg, vt, cands[:, 1], 0)
    w, scores = O.select(l, g)
    assert w >= 0 and scores[w] < 1.0
    if w == C - 1:  # keep room for a later duplicate: the winner moves to the front
        cands[0, 1, [0, w]] = cands[0, 1, [w, 0]]
        w = 0
    cands[0, 2] = cands[0, 1]
    cands[0, 2, C - 1] = cands[0, 2, w]
    picks = gm.acquire_requests(cands)
    assert picks.index[0, 0] == 0 and picks.score[0, 0] == 1.0
    for s in (1, 2):
        l, g = _oracle(gm, X, seg, vt, cands[:, s], 0)
        want, sc = O.select(l, g)
        assert want == w and picks.index[0, s] == want and picks.score[0, s] == sc[want]
        assert _same(picks.pdf_l[0, s], l[want]) and _same(picks.pdf_g[0, s], g[want])
    assert not picks.flags[0, 1] & NEAR_TIE and picks.near[0, 1] == 1
    assert picks.flags[0, 2] & NEAR_TIE and picks.near[0, 2] >= 2


@pytest.mark.parametrize("dc,du", [(5, 2), (24, 8)])
def test_one_request_is_the_one_request_call_byte_for_byte(device, dc, du):
    from hpbandster_amd import groups
    C = 64
    X, losses, seg, vt, levels, pool, kinds = _groups(dc, du, C)
    B = len(seg) - 1
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    a = gm.acquire(pool, sync=False).cpu().numpy()
    b = gm.acquire_requests(pool[:, None], sync=False).cpu().numpy()
    assert a.shape == (B, 48) and b.shape == (B, 1, 48)
    assert a.tobytes() == b.tobytes()


def _chain(device, dc, du, B, n_rows, S, C, seed):
    """hbx_seg_argsort_ex -> hbx_kde_fit -> hbx_kde_sample_groups (pool S C) -> hbx_kde_acquire_groups_batch through
    the C ABI on one non-default stream, nothing read on the host in between, twice."""
    import torch
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups, kde
    rs = np.random.RandomState(seed)
    D = dc + du
    lens = rs.randint(D + 2, n_rows + 1, size=B)
    lens[1] = D - 1  # a group without a model
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Nt = int(seg[-1])
    X = np.hstack([rs.rand(Nt, dc), rs.randint(0, 4, (Nt, du)).astype(np.float64)])
    losses = rs.rand(Nt)
    ng, nb = groups.group_sizes(lens, D)
    fg = np.array([kde.bandwidth_factor(int(v), D) if v else 0.0 for v in ng])
    fb = np.array([kde.bandwidth_factor(int(v), D) if v else 0.0 for v in nb])
    levels = np.array([0] * dc + [4] * du, dtype=np.int32)
    vt = np.array([0] * dc + [1] * du, dtype=np.int32)
    L = N.lib()
    st = torch.cuda.Stream(device=device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in dict(
        X=X, loss=losses, seg=seg, ng=ng, nb=nb, fg=fg, fb=fb, lv=levels, vt=vt).items()}
    order = torch.empty(Nt, dtype=torch.int64, device=device)
    sb = int(L.hbx_sort_scratch_bytes(Nt))
    scr = torch.empty(sb, dtype=torch.uint8, device=device)
    bw = [torch.zeros((B, D), dtype=torch.float64, device=device) for _ in range(2)]
    nl = [torch.zeros((B, D), dtype=torch.int32, device=device) for _ in range(2)]
    cands = torch.empty((B, S, C, D), dtype=torch.float64, device=device)
    derr = torch.empty((B, S, C), dtype=torch.uint8, device=device)
    wsb = int(L.hbx_kde_groups_batch_workspace_bytes(B, S, C, D))
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    res = torch.empty((B, S, 48), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)  # the inputs are in place; from here on one stream, no host read
    sh = st.cuda_stream
    out = []
    for _ in range(2):
        res.zero_()
        torch.cuda.synchronize(device)
        N.call("hbx_seg_argsort_ex", N.ptr(t["loss"]), N.ptr(t["seg"]), B, int(lens.max()), Nt, N.ptr(order),
               N.ptr(scr), sb, N.ORDER_NUMPY, sh)
        N.call("hbx_kde_fit", N.ptr(t["X"]), D, N.ptr(t["seg"]), B, N.ptr(order), N.ptr(t["ng"]), N.ptr(t["nb"]),
               N.ptr(t["fg"]), N.ptr(t["fb"]), N.ptr(t["vt"]), N.ptr(bw[0]), N.ptr(bw[1]), N.ptr(nl[0]), N.ptr(nl[1]),
               sh)
        N.call("hbx_kde_sample_groups", N.ptr(t["X"]), D, N.ptr(t["seg"]), B, N.ptr(order), N.ptr(t["ng"]),
               N.ptr(bw[0]), N.ptr(t["lv"]), 3.0, 77, 1000, 0, S * C, N.ptr(cands), N.ptr(derr), sh)
        N.call("hbx_kde_acquire_groups_batch", N.ptr(t["X"]), D, N.ptr(t["seg"]), B, N.ptr(order), N.ptr(t["ng"]),
               N.ptr(t["nb"]), N.ptr(t["vt"]), N.ptr(bw[0]), N.ptr(bw[1]), N.ptr(nl[0]), N.ptr(nl[1]), N.ptr(cands),
               S, C, N.ptr(res), N.ptr(ws), wsb, sh)
        st.synchronize()
        out.append((res.cpu().numpy().tobytes(), cands.cpu().numpy().copy()))
    host = dict(X=X, seg=seg, ng=ng, nb=nb, order=order.cpu().numpy(), bw=[b.cpu().numpy() for b in bw],
                nl=[v.cpu().numpy() for v in nl], vts="c" * dc + "u" * du)
    return out, host


@pytest.mark.parametrize("dc,du", [(5, 2), (24, 8)])
def test_device_chain_on_one_stream(device, dc, du):
    from oracle import c_oracle
    from hpbandster_amd import groups
    B, S, C = 12, 5, 64
    out, h = _chain(device, dc, du, B, 200, S, C, seed=11 + dc)
    (rec0, c0), (rec1, c1) = out
    assert rec0 == rec1  # a second identical run: identical bytes
    np.testing.assert_array_equal(c0, c1)
    picks = groups.GroupPicks.from_bytes(rec0, B, S)
    for b in range(B):
        if h["ng"][b] == 0:
            assert np.all(picks.index[b] == -1) and np.all(picks.flags[b] & NO_MODEL) and np.all(np.isnan(c0[b]))
            continue
        s0, e0 = h["seg"][b], h["seg"][b + 1]
        o = h["order"][s0:e0]
        Xb = h["X"][s0:e0]
        pool = c0[b].reshape(S * C, -1)
        with np.errstate(all="ignore"):
            l = c_oracle.kde_pdf(Xb[o[:h["ng"][b]]], h["bw"][0][b], h["vts"], h["nl"][0][b], pool, exact=True)
            g = c_oracle.kde_pdf(Xb[o[e0 - s0 - h["nb"][b]:]], h["bw"][1][b], h["vts"], h["nl"][1][b], pool, exact=True)
        for s in range(S):
            ls, gs = l[s * C:(s + 1) * C], g[s * C:(s + 1) * C]
            want, scores = O.select(ls, gs)
            assert picks.index[b, s] == want, (b, s, picks.index[b, s], want)
            if want >= 0:
                assert _same(picks.pdf_l[b, s], ls[want]) and _same(picks.pdf_g[b, s], gs[want]) and \
                    picks.score[b, s] == scores[want]


@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("dc,du", [(5, 2), (4, 2)])  # odd and even D
def test_sampler_requests_are_one_pool_of_s_times_c(device, dc, du, C):
    """sample(C, requests=S) == sample(S C) reshaped, rows and flags byte for byte: candidate (b, s, i) draws from
    the Philox counter counter_base + (b S + s) C + i."""
    from hpbandster_amd import groups
    rs = np.random.RandomState(3 + dc)
    B, D, S = 8, dc + du, 3
    lens = rs.randint(D + 2, 120, size=B)
    lens[2] = D  # no model
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Nt = int(seg[-1])
    X = np.hstack([rs.rand(Nt, dc), rs.randint(0, 3, (Nt, du)).astype(np.float64)])
    X[seg[5]:seg[6], 1] = 0.0  # bandwidth 0 at the bound: every draw of that dim is a domain error
    gm = groups.fit_groups(X, rs.rand(Nt), seg, "c" * dc + "u" * du, device=device)
    levels = [0] * dc + [3] * du
    c4, e4 = gm.sample(C, seed=9, levels=levels, counter_base=12345, requests=S)
    c3, e3 = gm.sample(S * C, seed=9, levels=levels, counter_base=12345)
    assert tuple(c4.shape) == (B, S, C, D) and tuple(e4.shape) == (B, S, C)
    assert tuple(c3.shape) == (B, S * C, D)
    assert c4.cpu().numpy().tobytes() == c3.cpu().numpy().tobytes()
    assert e4.cpu().numpy().tobytes() == e3.cpu().numpy().tobytes()
    assert e3.cpu().numpy().any()


def test_python_surface_and_edges(device):
    import torch
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    from hpbandster_amd import synthetic as S_
    dc, du, D = 4, 2, 6
    lens = np.array([40, 3, 90, 6, 64])  # groups 1 and 3: rows <= D, no model
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = S_.make_observations(int(seg[-1]), dc, du, 3, seed=5)
    losses = S_.make_losses(int(seg[-1]), seed=6)
    vts, lv = S_.var_type_string(dc, du), [0] * dc + [3] * du
    gm = groups.fit_groups(X, losses, seg, vts, device=device)
    rows, picks = gm.propose(32, seed=4, levels=lv, requests=4)
    assert rows.shape == (5, 4, D) and len(picks) == 5
    for name in groups.GroupPicks.__slots__:
        assert getattr(picks, name).shape == (5, 4), name
    np.testing.assert_array_equal(np.isnan(rows).all(axis=2), picks.index < 0)
    np.testing.assert_array_equal(np.isnan(rows).any(axis=2), picks.index < 0)
    np.testing.assert_array_equal(picks.index < 0, np.repeat(~gm.has_model[:, None], 4, axis=1))
    cands, _ = gm.sample(32, seed=4, levels=lv, requests=4)
    ch = cands.cpu().numpy()
    for b in (0, 2, 4):
        for s in range(4):
            np.testing.assert_array_equal(rows[b, s], ch[b, s, picks.index[b, s]])
    assert gm.acquire_requests(cands, sync=False).shape == (5, 4, 48)
    np.testing.assert_array_equal(gm.acquire_requests(ch).index, picks.index)  # a host pool
    # requests=None: today's shapes
    r1, p1 = gm.propose(32, seed=4, levels=lv)
    assert r1.shape == (5, D) and p1.index.shape == (5,)
    # S = 0 and C = 0 are legal
    p0 = gm.acquire_requests(np.empty((5, 0, 8, D)))
    assert len(p0) == 5 and p0.index.shape == (5, 0)
    pc = gm.acquire_requests(np.empty((5, 3, 0, D)))
    assert pc.index.shape == (5, 3) and np.all(pc.index == -1) and np.all(np.isnan(pc.score)) and \
        np.all(np.isnan(pc.pdf_l)) and np.all(pc.flags == 0)
    assert gm.sample(0, 1, lv, requests=3)[0].shape == (5, 3, 0, D)
    rz, pz = gm.propose(8, 1, lv, requests=0)
    assert rz.shape == (5, 0, D) and pz.index.shape == (5, 0)
    # B = 0 is legal
    g0 = groups.fit_groups(np.empty((0, D)), np.empty(0), np.zeros(1, np.int64), vts, device=device)
    r0, pk0 = g0.propose(8, 1, lv, requests=3)
    assert r0.shape == (0, 3, D) and len(pk0) == 0 and pk0.index.shape == (0, 3)
    # B * S * C past int32: the size helper says -1 and the call is an argument error
    L = N.lib()
    assert L.hbx_kde_groups_batch_workspace_bytes(1 << 12, 1 << 10, 1 << 10, D) == -1
    assert L.hbx_kde_groups_batch_workspace_bytes(5, 4, 32, D) == 256 + 5 * 4 * 32 * 16
    assert gm.workspace_bytes(32, 4) == 256 + 5 * 4 * 32 * 16 and gm.workspace_bytes(32) == 256 + 5 * 32 * 16
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=device)
    res = torch.empty((5, 4, 48), dtype=torch.uint8, device=device)

    def call(B, S, C, wsb):
        model = tuple(B if name == "B" else arg for name, arg in zip(groups.MODEL_ARGS, gm.model_args()))
        return L.hbx_kde_acquire_groups_batch(*model, N.ptr(cands), S, C, N.ptr(res), N.ptr(ws), wsb, None)

    assert call(1 << 12, 1 << 10, 1 << 10, 1 << 12) == -1 and b"int32" in L.hbx_last_error()  # (checked first)
    assert call(5, 4, 32, 1 << 12) == -1 and b"workspace too small" in L.hbx_last_error()
    with pytest.raises(N.HbxError):
        gm.acquire_requests(cands, workspace=ws)
