"""Grouped successive halving on the GPU: hbx_sh_advance_groups against a numpy restatement of its contract (byte
equality, guard regions around every output), and GroupSuccessiveHalving / GroupHyperband against a loop written
here from the public pieces and against the host SuccessiveHalving class."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# csrc/hbx_groups_sh.hip: positions per ranking step, per tile, the longest one-workgroup bracket, and the block
# budget that decides the slice count of longer ones (B > SH_BLOCKS / 2: one workgroup per bracket at any length)
SH_SUB, SH_TILE, SH_S1, SH_BLOCKS = 256, 1024, 8192, 2048
QNAN = np.uint64(0x7FF8000000000000)
NONE = -2 ** 31
GUARD = 64  # sentinel elements before and after each output
S_ROWS, S_SRC, S_CNT = 0x5EED5EED5EED5EED, 0x5A5A5A5A, 0x1DEA1DEA1DEA1DEA

LENGTHS = [0, 1, 63, 64, 65, 0, 255, 256, 257, 1023, 1024, 1025, 0, 0, SH_SUB - 1, SH_SUB + 1, SH_TILE - 1,
           SH_TILE + 1, SH_S1 - 1, SH_S1, SH_S1 + 1, 0]
MASKS = ["clear", "set", "first", "last", "alternating", "p0.01", "p0.33", "p0.9", "value2", "value255"]


def _restate(rows, seg, mask, fresh, K):
    """the contract, on uint64 bit patterns: rows [N, D], mask [N], fresh None or [B, F, D]"""
    B, D = len(seg) - 1, rows.shape[1]
    out = np.full((B, K, D), QNAN, dtype=np.uint64)
    src = np.full((B, K), NONE, dtype=np.int32)
    counts = np.zeros((B, 2), dtype=np.int64)
    for b in range(B):
        pos = np.nonzero(mask[seg[b]:seg[b + 1]])[0]
        na = min(len(pos), K)
        out[b, :na] = rows[seg[b] + pos[:na]]
        src[b, :na] = pos[:na]
        f = 0 if fresh is None else min(fresh.shape[1], K - na)
        if f:
            out[b, na:na + f] = fresh[b, :f]
            src[b, na:na + f] = -1 - np.arange(f)
        counts[b] = (len(pos), f)
    return out, src, counts


def _mask(kind, seg, rs):
    n = int(seg[-1])
    m = np.zeros(n, dtype=np.uint8)
    if kind == "set":
        m[:] = 1
    elif kind == "first":
        m[seg[:-1][np.diff(seg) > 0]] = 1
    elif kind == "last":
        m[seg[1:][np.diff(seg) > 0] - 1] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind.startswith("p"):
        m[rs.rand(n) < float(kind[1:])] = 1
    elif kind.startswith("value"):
        m[rs.rand(n) < 0.5] = int(kind[5:])
    return m


def _bits(rs, shape):
    """random 64-bit patterns: NaNs of every payload, infinities, subnormals and both zeros' neighbours among them"""
    return np.frombuffer(rs.bytes(8 * int(np.prod(shape))), dtype=np.uint64).reshape(shape).copy()


def _dev_f64(torch, device, bits, off8):
    """the patterns as a float64 device tensor starting 0 or 8 bytes into an allocation"""
    buf = torch.empty(bits.size + 2, dtype=torch.int64, device=device)  # (allocations are at least 16-byte aligned)
    lo = 1 if off8 else 0
    view = buf[lo:lo + bits.size]
    view.copy_(torch.from_numpy(bits.view(np.int64).reshape(-1)))
    t = view.view(torch.float64).view(bits.shape)
    assert bits.size == 0 or t.data_ptr() % 16 == (8 if off8 else 0)
    return t


class _Guarded(object):
    """the three outputs inside sentinel-filled buffers"""

    def __init__(self, torch, device, B, K, D, off8):
        g = GUARD + (1 if off8 else 0)
        self.g = g
        self.rbuf = torch.full((g + B * K * D + GUARD,), S_ROWS, dtype=torch.int64, device=device)
        self.sbuf = torch.full((GUARD + B * K + GUARD,), S_SRC, dtype=torch.int32, device=device)
        self.cbuf = torch.full((GUARD + B * 2 + GUARD,), S_CNT, dtype=torch.int64, device=device)
        self.rows = self.rbuf[g:g + B * K * D].view(torch.float64).view(B, K, D)
        self.src = self.sbuf[GUARD:GUARD + B * K].view(B, K)
        self.counts = self.cbuf[GUARD:GUARD + B * 2].view(B, 2)
        assert self.rows.data_ptr() % 16 == (8 if off8 else 0)
        self.shape = (B, K, D)

    def out(self):
        return self.rows, self.src, self.counts

    def fetch(self):
        """(rows as uint64 [B, K, D], src, counts) after checking the guards"""
        B, K, D = self.shape
        r, s, c = self.rbuf.cpu().numpy(), self.sbuf.cpu().numpy(), self.cbuf.cpu().numpy()
        g = self.g
        assert np.all(r[:g] == S_ROWS) and np.all(r[g + B * K * D:] == S_ROWS), "rows_out guard"
        assert np.all(s[:GUARD] == S_SRC) and np.all(s[GUARD + B * K:] == S_SRC), "src_out guard"
        assert np.all(c[:GUARD] == S_CNT) and np.all(c[GUARD + 2 * B:] == S_CNT), "counts_out guard"
        return (r[g:g + B * K * D].view(np.uint64).reshape(B, K, D), s[GUARD:GUARD + B * K].reshape(B, K),
                c[GUARD:GUARD + 2 * B].reshape(B, 2))


def _check(torch, device, rows_b, rows_d, seg, seg_d, mask, fresh_b, fresh_d, K, off8, tag):
    from hpbandster_amd import groups
    B, D = len(seg) - 1, rows_b.shape[1]
    G = _Guarded(torch, device, B, K, D, off8)
    md = torch.from_numpy(mask).to(device)
    got = groups.advance(rows_d, seg_d, md, K, fresh=fresh_d, sync=False, out=G.out())
    assert got[0].data_ptr() == G.rows.data_ptr()
    r, s, c = G.fetch()
    wr, ws, wc = _restate(rows_b, seg, mask, fresh_b, K)
    assert c.tobytes() == wc.tobytes(), (tag, "counts", c[:4], wc[:4])
    assert s.tobytes() == ws.tobytes(), (tag, "src", np.argwhere(s != ws)[:4])
    assert r.tobytes() == wr.tobytes(), (tag, "rows", np.argwhere(r != wr)[:4])


@pytest.mark.parametrize("D,off8", [(1, False), (2, False), (2, True), (3, False), (32, False), (32, True),
                                    (33, False), (256, False), (256, True)])
def test_kernel_equals_restatement(device, D, off8):
    """every bracket length at which a path changes, mixed with empty brackets, in one call; every mask kind; K = 1,
    K below most set counts, K above set + F; fresh absent, F = 0, F below and above the deficit"""
    import torch
    rs = np.random.RandomState(1000 + D)
    seg = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)
    B, n = len(LENGTHS), int(seg[-1])
    rows_b = _bits(rs, (n, D))
    rows_d = _dev_f64(torch, device, rows_b, off8)
    seg_d = torch.from_numpy(seg).to(device)
    fresh = {}
    for F in (0, 3, 40):
        fb = _bits(rs, (B, F, D))
        fresh[F] = (fb, _dev_f64(torch, device, fb, off8))
    for kind in MASKS:
        mask = _mask(kind, seg, rs)
        for K, F in ((1, None), (1, 3), (37, 0), (37, 3), (37, 40), (300, None), (300, 40)):
            fb, fd = (None, None) if F is None else fresh[F]
            _check(torch, device, rows_b, rows_d, seg, seg_d, mask, fb, fd, K, off8, (D, off8, kind, K, F))


@pytest.mark.parametrize("between", [False, True])
def test_long_bracket_takes_the_sliced_route(device, between):
    """one bracket of 70 000 at D = 3 -- count, rank and gather launches --, alone and between short brackets"""
    import torch
    rs = np.random.RandomState(7)
    lens = [5, 0, 70000, 300, 0] if between else [70000]
    seg = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    B, n, D = len(lens), int(seg[-1]), 3
    rows_b = _bits(rs, (n, D))
    rows_d = _dev_f64(torch, device, rows_b, False)
    seg_d = torch.from_numpy(seg).to(device)
    fb = _bits(rs, (B, 50, D))
    fd = _dev_f64(torch, device, fb, False)
    for kind in ("p0.33", "set", "last", "clear", "p0.01"):
        mask = _mask(kind, seg, rs)
        for K, fresh in ((1, False), (100, True), (30000, True), (70001, False)):
            _check(torch, device, rows_b, rows_d, seg, seg_d, mask, fb if fresh else None, fd if fresh else None, K,
                   False, (between, kind, K, fresh))


def test_many_brackets_one_workgroup_each(device):
    """B > SH_BLOCKS / 2: no sliced route, a workgroup walks a bracket longer than SH_S1 by itself"""
    import torch
    rs = np.random.RandomState(11)
    lens = rs.randint(0, 6, size=SH_BLOCKS // 2 + 1)
    lens[500] = SH_S1 + 1000
    seg = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    B, n, D = len(lens), int(seg[-1]), 2
    rows_b = _bits(rs, (n, D))
    rows_d = _dev_f64(torch, device, rows_b, False)
    fb = _bits(rs, (B, 2, D))
    fd = _dev_f64(torch, device, fb, False)
    _check(torch, device, rows_b, rows_d, seg, torch.from_numpy(seg).to(device), _mask("p0.33", seg, rs), fb, fd, 4,
           False, "many")


def test_payloads_come_back_bit_for_bit(device):
    import torch
    from hpbandster_amd import groups
    special = np.array([0x7FF8000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000001, 0xFFF0000000000000,
                        0x7FF0000000000000, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
                        0x7FF8000000000000, 0x3FF0000000000000], dtype=np.uint64)
    rows_b = np.stack([np.roll(special, i) for i in range(10)])[:, :4].copy()  # [10, 4]
    fresh_b = special[::-1][:8].reshape(1, 2, 4).copy()
    seg = np.array([0, 10], dtype=np.int64)
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1], dtype=np.uint8)
    for off8 in (False, True):
        rows_d, fresh_d = _dev_f64(torch, device, rows_b, off8), _dev_f64(torch, device, fresh_b, off8)
        r, s, c = groups.advance(rows_d, torch.from_numpy(seg).to(device), torch.from_numpy(mask).to(device), 10,
                                 fresh=fresh_d)
        wr, ws, wc = _restate(rows_b, seg, mask, fresh_b, 10)
        assert r.view(np.uint64).tobytes() == wr.tobytes() and s.tobytes() == ws.tobytes()
        assert c.tolist() == [[7, 2]] and s[0, -1] == NONE and np.all(r.view(np.uint64)[0, -1] == QNAN)


def test_host_arrays_and_bool_masks(device):
    from hpbandster_amd import groups
    rs = np.random.RandomState(3)
    rows = rs.rand(12, 3)
    seg = np.array([0, 5, 5, 12])
    mask = rs.rand(12) < 0.5
    r, s, c = groups.advance(rows, seg, mask, 4, device=device)
    wr, ws, wc = _restate(rows.view(np.uint64), seg, mask, None, 4)
    assert r.view(np.uint64).tobytes() == wr.tobytes() and s.tobytes() == ws.tobytes() and c.tobytes() == wc.tobytes()
    assert r.shape == (3, 4, 3) and s.dtype == np.int32 and c.dtype == np.int64


def test_edges_and_errors(device):
    import torch
    from hpbandster_amd import groups
    from hpbandster_amd import _native as N
    rows = torch.zeros((8, 3), dtype=torch.float64, device=device)
    mask = torch.ones(8, dtype=torch.uint8, device=device)
    seg = torch.tensor([0, 8], dtype=torch.int64, device=device)
    fresh = torch.zeros((1, 2, 3), dtype=torch.float64, device=device)
    # K == 0 and B == 0: success, outputs untouched
    G = _Guarded(torch, device, 1, 4, 3, False)
    L = N.lib()
    N.check(L.hbx_sh_advance_groups(N.ptr(rows), 3, N.ptr(seg), 1, N.ptr(mask), None, 0, 0, N.ptr(G.rows),
                                    N.ptr(G.src), N.ptr(G.counts), None))
    N.check(L.hbx_sh_advance_groups(N.ptr(rows), 3, N.ptr(seg), 0, N.ptr(mask), None, 0, 4, N.ptr(G.rows),
                                    N.ptr(G.src), N.ptr(G.counts), None))
    torch.cuda.synchronize(device)
    assert np.all(G.rbuf.cpu().numpy() == S_ROWS) and np.all(G.sbuf.cpu().numpy() == S_SRC)
    assert np.all(G.cbuf.cpu().numpy() == S_CNT)
    r, s, c = groups.advance(rows, seg, mask, 0)
    assert r.shape == (1, 0, 3) and s.shape == (1, 0) and c.shape == (1, 2)
    r, s, c = groups.advance(rows[:0], seg[:1], mask[:0], 4)
    assert r.shape == (0, 4, 3) and s.shape == (0, 4)

    def call(rows_p=N.ptr(rows), D=3, seg_p=N.ptr(seg), B=1, mask_p=N.ptr(mask), fresh_p=N.ptr(fresh), F=2, K=4,
             out_p=N.ptr(G.rows), src_p=N.ptr(G.src)):
        N.check(L.hbx_sh_advance_groups(rows_p, D, seg_p, B, mask_p, fresh_p, F, K, out_p, src_p, N.ptr(G.counts),
                                        None))

    for bad in (dict(rows_p=None), dict(seg_p=None), dict(mask_p=None), dict(out_p=None), dict(src_p=None),
                dict(D=0), dict(D=257), dict(B=-1), dict(K=-1), dict(F=-1), dict(fresh_p=None, F=2)):
        with pytest.raises(N.HbxError):
            call(**bad)
    torch.cuda.synchronize(device)
    assert np.all(G.rbuf.cpu().numpy() == S_ROWS)  # refused before anything was launched
    with pytest.raises(N.HbxError):
        groups.advance(rows, seg, mask, 4, fresh=torch.zeros((2, 2, 3), dtype=torch.float64, device=device))
    with pytest.raises(N.HbxError):
        groups.advance(rows, seg, mask[:5], 4)


def test_asynchronous_use(device):
    """two calls queued on a side stream, device tensors in and out, compared after the stream's synchronisation"""
    import torch
    from hpbandster_amd import groups
    rs = np.random.RandomState(5)
    lens = [1000] * 6 + [SH_S1 + 5]
    seg = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    B, n, D, K = len(lens), int(seg[-1]), 32, 333
    rows_b, fresh_b = _bits(rs, (n, D)), _bits(rs, (B, K, D))
    m1, m2 = _mask("p0.33", seg, rs), _mask("p0.01", seg, rs)
    rows_d, fresh_d = _dev_f64(torch, device, rows_b, False), _dev_f64(torch, device, fresh_b, False)
    seg_d, d1, d2 = (torch.from_numpy(a).to(device) for a in (seg, m1, m2))
    torch.cuda.synchronize(device)
    st = torch.cuda.Stream(device=device)
    a = groups.advance(rows_d, seg_d, d1, K, fresh=fresh_d, stream=st, sync=False)
    b = groups.advance(a[0].view(B * K, D), torch.arange(B + 1, device=device) * K, d2[:B * K], 100, stream=st,
                       sync=False)  # queued behind a, reading a's rows
    for out in (a, b):
        assert all(t.is_cuda for t in out)
    st.synchronize()
    wa = _restate(rows_b, seg, m1, fresh_b, K)
    wb = _restate(wa[0].reshape(B * K, D), np.arange(B + 1) * K, m2[:B * K], None, 100)
    for got, want in ((a, wa), (b, wb)):
        assert got[0].cpu().numpy().view(np.uint64).tobytes() == want[0].tobytes()
        assert got[1].cpu().numpy().tobytes() == want[1].tobytes()
        assert got[2].cpu().numpy().tobytes() == want[2].tobytes()


# ---- the driver -------------------------------------------------------------------------------------------------
B_RUNS, C_SAMPLES = 3, 16
# seed 6: 7 of run 1's 9 prior draws of iteration 0 have x0 > 0.5 (hbx_kde_finish_groups' prior, restated on the host
# by tests/test_gpu_groups_config.py's _prior_row), so the crash rule below leaves run 1 one survivor short
KW = dict(var_type="ccu", levels=[0, 0, 4], num_samples=C_SAMPLES, seed=6)


def _loss(rows):  # tests/test_gpu_groups_config.py's quadratic
    return ((rows[..., 0] - 0.3) ** 2 + (rows[..., 1] - 0.7) ** 2 + 0.1 * rows[..., 2])


def _plain(rows, budget):
    return _loss(rows) / budget


def _quantised(rows, budget):  # three levels: ties straddle the k-th place
    return np.clip(np.floor(_loss(rows) * 4.0), 0.0, 2.0)


def _crash1(rows, budget):  # run 1's configurations with x0 > 0.5 crash at budget 1
    out = _plain(rows, budget)
    if budget == 1.0:
        out[1, rows[1, :, 0] > 0.5] = np.inf
    return out


def _crash_all(rows, budget):  # run 1's whole first stage crashes
    out = _plain(rows, budget)
    if budget == 1.0:
        out[1, :] = np.inf
    return out


def _objective(f):
    """the host function as a driver objective (computed on the host so that the loop below sees the same bits)"""
    def objective(rows, budget, info):
        assert rows.is_cuda and info["budget"] == budget
        return f(rows.cpu().numpy(), budget)
    return objective


_RUNS = {}


def _driver(device, name, rate=None):
    """one GroupHyperband run of 3 iterations per (objective, resampling rate), shared by the tests"""
    from hpbandster_amd import groups
    key = (name, rate)
    if key not in _RUNS:
        opt = groups.GroupBOHB(B_RUNS, device=device, **KW)
        kw = {} if rate is None else dict(resampling_rate=rate)
        hb = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9, **kw)
        _RUNS[key] = (hb.run(3, _objective(globals()[name])), opt)
    return _RUNS[key]


def _loop(device, f, rate=None):
    """the same run from the public pieces: get_configs / new_results, the host mask of promote_segments, numpy
    compaction, and the counter rule spelled out"""
    from hpbandster_amd import groups, promote
    from hpbandster_amd.HB_master import hb_budgets, hb_bracket
    opt = groups.GroupBOHB(B_RUNS, device=device, **KW)
    B, D = B_RUNS, 3
    max_sh, budgets = hb_budgets(3, 1, 9)
    counter, out = 0, []
    for it in range(3):
        s, ns = hb_bracket(it, 3, max_sh)
        bud = [float(v) for v in budgets[-s - 1:]]
        cfg = opt.get_configs(bud[0], S=ns[0], counter_base=counter)
        counter += B * ns[0] * C_SAMPLES
        rows, src = cfg.rows, np.tile(-1 - np.arange(ns[0], dtype=np.int32), (B, 1))
        for stage, n in enumerate(ns):
            losses = f(rows, bud[stage])
            out.append((it, stage, bud[stage], rows, losses, src))
            opt.new_results(bud[stage], rows, losses)
            if stage == len(ns) - 1:
                break
            K = ns[stage + 1]
            k = K if rate is None else max(1, K * (1 - rate))
            seg = np.arange(B + 1, dtype=np.int64) * n
            mask = promote.promote_segments(losses.reshape(-1), seg, [k] * B, device=device)
            base = counter
            counter += B * K * C_SAMPLES  # reserved whether the fills are computed or not
            fresh = None
            if np.any(mask.reshape(B, n).sum(axis=1) < K):
                fresh = opt.get_configs(bud[stage + 1], S=K, counter_base=base).rows
            r, src, _ = _restate(rows.reshape(B * n, D).view(np.uint64), seg, mask,
                                 None if fresh is None else fresh.view(np.uint64), K)
            rows = r.view(np.float64)
    return out


@pytest.mark.parametrize("name,rate", [("_plain", None), ("_quantised", None), ("_crash1", None), ("_plain", 0.5)])
def test_driver_equals_the_loop(device, name, rate):
    res, _ = _driver(device, name, rate)
    want = _loop(device, globals()[name], rate)
    assert [(r.iteration, r.stage, r.budget, r.rows.shape) for r in res.stages] == \
        [(it, st, b, rows.shape) for it, st, b, rows, _, _ in want]
    assert [r.rows.shape[1] for r in res.stages] == [9, 3, 1, 3, 1, 3]
    for r, (it, st, b, rows, losses, src) in zip(res.stages, want):
        assert r.rows.tobytes() == rows.tobytes(), (it, st)
        assert r.losses.tobytes() == np.asarray(losses, dtype=np.float64).tobytes(), (it, st)
        assert r.src.tobytes() == src.tobytes(), (it, st)
        assert r.model_based.shape == r.src.shape and r.model_based.dtype == bool
    # the run crosses the no-model -> model boundary at budget 1: stage 0 of iteration 0 is all prior draws, and
    # iteration 1 is proposed by a model
    assert not res[(0, 0)].model_based.any() and res[(1, 0)].model_based.any()


class _Job(object):
    def __init__(self, cid, config, budget, loss):
        self.id, self.kwargs = cid, dict(config=config, budget=budget)
        self.result, self.timestamps, self.exception = {"loss": loss}, {}, None


def _host_class_orders(cls, ns, bud, losses_of_stage):
    """One bracket through the host iteration class, fed ``losses_of_stage[s]`` in run order: per stage the config
    ids in the order the class runs them."""
    fresh = iter(range(10 ** 6))
    sh = cls(0, ns, bud, lambda budget: ({"fresh": next(fresh)}, {}))
    orders = []
    for s in range(len(ns)):
        runs = []
        while True:
            nxt = sh.get_next_run()
            if nxt is None:
                break
            runs.append(nxt)
            if len(runs) == ns[s]:
                break
        assert len(runs) == ns[s]
        orders.append([cid for cid, _, _ in runs])
        for (cid, config, budget), loss in zip(runs, losses_of_stage[s]):
            assert budget == bud[s]
            sh.register_result(_Job(cid, config, budget, float(loss)))
    assert sh.get_next_run() is None and sh.is_finished
    return orders


@pytest.mark.parametrize("name,rate", [("_plain", None), ("_quantised", None), ("_crash1", None), ("_plain", 0.5),
                                       ("_quantised", 0.5)])
def test_survivors_equal_the_host_class(device, name, rate):
    """per run and stage: which configurations advance, and in which order, as SuccessiveHalving /
    SuccessiveResampling (pinned to the reference by the golden fixtures) decide from the same losses"""
    from hpbandster_amd.HB_iteration import SuccessiveHalving, SuccessiveResampling
    res, _ = _driver(device, name, rate)
    cls = SuccessiveHalving if rate is None else SuccessiveResampling
    ladders = {0: ([9, 3, 1], [1.0, 3.0, 9.0]), 1: ([3, 1], [3.0, 9.0]), 2: ([3], [9.0])}
    for it, (ns, bud) in ladders.items():
        for b in range(B_RUNS):
            orders = _host_class_orders(cls, ns, bud, [res[(it, s)].losses[b] for s in range(len(ns))])
            for s in range(1, len(ns)):
                src = res[(it, s)].src[b]
                for j, cid in enumerate(orders[s]):
                    if src[j] >= 0:
                        assert cid == orders[s - 1][src[j]], (it, b, s, j)
                    else:
                        assert cid not in orders[s - 1] and src[j] != NONE, (it, b, s, j)
                if rate is not None:  # HB_iteration.py:242: ceil(max(1, n (1 - rate))) advance, the rest are fills
                    assert int((src >= 0).sum()) == int(np.ceil(max(1, ns[s] * (1 - rate)))), (it, b, s)
                    assert int((src < 0).sum()) == ns[s] - int((src >= 0).sum())


def test_runs_are_independent(device):
    """run 1's crashes leave runs 0 and 2 byte for byte as they are without them"""
    crash, _ = _driver(device, "_crash1")
    plain, _ = _driver(device, "_plain")
    for rc, rp in zip(crash.stages, plain.stages):
        for b in (0, 2):
            assert rc.rows[b].tobytes() == rp.rows[b].tobytes(), (rc.iteration, rc.stage, b)
            assert rc.losses[b].tobytes() == rp.losses[b].tobytes() and rc.src[b].tobytes() == rp.src[b].tobytes()


@pytest.mark.parametrize("name", ["_crash1", "_crash_all"])
def test_fills_are_the_reserved_requests(device, name):
    """a deficit's slots hold requests (b, i) of the block of counters the transition reserved; a stage that crashes
    entirely is followed by one made only of fills (HB_iteration.py:172)"""
    import torch
    from hpbandster_amd import groups
    f = globals()[name]
    opt = groups.GroupBOHB(B_RUNS, device=device, **KW)
    sh = groups.GroupSuccessiveHalving([9, 3, 1], [1.0, 3.0, 9.0])
    cfg = opt.get_configs(1.0, S=9, sync=False)
    assert opt.counter == B_RUNS * 9 * C_SAMPLES
    rows_h = cfg.rows.cpu().numpy()
    losses = f(rows_h, 1.0)
    crashed = ~np.isfinite(losses[1])
    assert crashed.sum() > 6  # fewer than 3 of run 1's 9 survive (the seed's premise, see KW)
    st = sh.step(opt, cfg.rows, torch.from_numpy(losses).to(device), 0)
    assert st.counter_base == B_RUNS * 9 * C_SAMPLES and opt.counter == st.counter_base + B_RUNS * 3 * C_SAMPLES
    want = opt.get_configs(3.0, S=3, counter_base=st.counter_base)  # the model is as the fills saw it
    rows, src, counts = st.rows.cpu().numpy(), st.src.cpu().numpy(), st.counts.cpu().numpy()
    n_ok = int((~crashed).sum())
    assert counts[1].tolist() == [n_ok, 3 - n_ok] and counts[0].tolist() == [3, 0] and counts[2].tolist() == [3, 0]
    assert np.all(src[[0, 2]] >= 0) and (src[1] < 0).sum() == 3 - n_ok
    if name == "_crash_all":
        assert src[1].tolist() == [-1, -2, -3]
    for j in range(3):
        if src[1, j] < 0:
            assert rows[1, j].tobytes() == want.rows[1, -1 - src[1, j]].tobytes(), j
        else:
            assert rows[1, j].tobytes() == rows_h[1, src[1, j]].tobytes(), j


def test_incumbent_and_keep_modes(device):
    import torch
    from hpbandster_amd import groups
    res, _ = _driver(device, "_crash1")
    budget, loss, row = res.incumbent()
    for b in range(B_RUNS):
        at = [r for r in res.stages if np.isfinite(r.losses[b]).any()]
        top = max(r.budget for r in at)
        ls = np.concatenate([np.where(np.isfinite(r.losses[b]), r.losses[b], np.inf) for r in at if r.budget == top])
        rs = np.concatenate([r.rows[b] for r in at if r.budget == top])
        i = int(np.argmin(ls))
        assert budget[b] == top == 9.0 and loss[b] == ls[i] and row[b].tobytes() == rs[i].tobytes()
    opt = groups.GroupBOHB(B_RUNS, device=device, **KW)
    dev = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9).run(3, _objective(_crash1), keep="device")
    assert all(isinstance(getattr(r, a), torch.Tensor) and getattr(r, a).is_cuda for r in dev.stages
               for a in ("rows", "losses", "src", "model_based"))
    assert all(t.is_cuda for t in dev.incumbent())
    for r, h in zip(dev.stages, res.stages):
        assert r.rows.cpu().numpy().tobytes() == h.rows.tobytes() and r.src.cpu().numpy().tobytes() == h.src.tobytes()
        assert r.model_based.cpu().numpy().tobytes() == h.model_based.tobytes()
    opt = groups.GroupBOHB(B_RUNS, device=device, **KW)
    only = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9).run(3, _objective(_crash1), keep=None)
    assert only.stages == [] and len(only) == 0
    for got, want in zip(only.incumbent(), res.incumbent()):
        assert isinstance(got, np.ndarray) and got.tobytes() == want.tobytes()
