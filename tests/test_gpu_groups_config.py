"""Grouped get_config (hbx_kde_finish_groups / hbx_kde_propose_groups, GroupModel.get_config / finish,
groups.sample_prior, GroupBOHB) on the GPU.  Every check is a byte equality against a host restatement of the rule
in include/hbx.h: the library's host Philox function for the request's decision and prior draws, the table of
source codes for the rest."""
import math

import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import NO_MODEL, UNSUPPORTED, _oracle, _same

pytestmark = pytest.mark.gpu

MODEL, RANDOM_FRACTION, SRC_NO_MODEL, NO_SCORE, DOMAIN_ERR = 0, 1, 2, 3, 4
DECIDE_WORD, PRIOR_WORD0 = 0xFFFFFFFE, 0xFFFE0000
SHAPES = [(1, 0), (5, 2), (4, 2), (24, 8), (40, 30)]


# ---- the host restatement ------------------------------------------------------------------------------------
def _philox(seed, i, word, stream):
    from hpbandster_amd import _native as N
    c = np.array([i & 0xFFFFFFFF, (i >> 32) & 0xFFFFFFFF, word, stream], dtype=np.uint32)
    k = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    o = np.zeros(4, dtype=np.uint32)
    N.check(N.lib().hbx_philox4x32_10(N.ptr(c), N.ptr(k), N.ptr(o)))
    return [int(v) for v in o]


def _u01(r, w):
    bits = (r[2 * w] << 32) | r[2 * w + 1]
    return (float(bits >> 11) + 0.5) * 2.0 ** -53


def _decision(seed, ctr, stream=0):
    return _u01(_philox(seed, ctr, DECIDE_WORD, stream), 0)


def _prior_row(levels, seed, ctr, stream=0):
    row = np.empty(len(levels))
    for p in range((len(levels) + 1) // 2):
        r = _philox(seed, ctr, PRIOR_WORD0 + p, stream)
        for w in (0, 1):
            d = 2 * p + w
            if d < len(levels):
                u, t = _u01(r, w), int(levels[d])
                row[d] = u if t == 0 else float(min(t - 1, int(math.floor(t * u))))
    return row


def _restate(rec, cands, err, levels, C, rf, seed, cb, Q, stream=0):
    """(rows [Q, D], source [Q]) of Q requests: ``rec`` the Q records (groups.RECORD) or None, ``cands`` [Q, C, D],
    ``err`` [Q, C] or None"""
    rows = np.empty((Q, len(levels)))
    source = np.empty(Q, dtype=np.uint8)
    for q in range(Q):
        ctr = cb + q * C
        if rec is None or rec["flags"][q] & (NO_MODEL | UNSUPPORTED):
            s = SRC_NO_MODEL
        elif _decision(seed, ctr, stream) < rf:
            s = RANDOM_FRACTION
        elif err is not None and err[q].any():
            s = DOMAIN_ERR
        elif rec["index"][q] < 0:
            s = NO_SCORE
        else:
            s = MODEL
        source[q] = s
        rows[q] = cands[q, rec["index"][q]] if s == MODEL else _prior_row(levels, seed, ctr, stream)
    return rows, source


def _records(t):
    from hpbandster_amd import groups
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=groups.RECORD)


# ---- six groups: two with models, one too small, one empty, one unsupported, one whose pool will be NaN ------------
_CACHE = {}


def _six(device, dc, du):
    from hpbandster_amd import groups
    if (dc, du) not in _CACHE:
        rs = np.random.RandomState(1000 * dc + du)
        D = dc + du
        levels = [0] * dc + [int(v) for v in rs.randint(2, 7, size=du)]
        lens = np.array([3 * D + 20, 2 * D + 9, D, 0, 2 * D + 12, 2 * D + 30])
        seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(seg[-1])
        X = np.empty((n, D))
        X[:, :dc] = rs.rand(n, dc)
        for u in range(du):
            X[:, dc + u] = rs.randint(0, levels[dc + u], size=n)
        kinds = {2: "no_model", 3: "no_model", 5: "nan_pool"}
        if du:
            X[seg[4]:seg[5], dc] += 0.5  # non-integer categorical codes: unsupported
            kinds[4] = "unsupported"
        vt = "c" * dc + "u" * du
        losses = rs.rand(n)
        gm = groups.fit_groups(X, losses, seg, vt, device=device)
        np.testing.assert_array_equal(gm.has_model, [True, True, False, False, True, True])
        _CACHE[(dc, du)] = (gm, X, seg, vt, levels, kinds)
    return _CACHE[(dc, du)]


@pytest.mark.parametrize("C", [1, 37, 65])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dc,du", SHAPES)
def test_finish_equals_the_restatement(device, dc, du, S, C):
    """(4, 2): an even D; (40, 30): D = 70, a second 64-lane pass; C = 65: a second pass over the error bytes.  The
    three fractions share one acquisition; over them every source code occurs."""
    gm, X, seg, vt, levels, kinds = _six(device, dc, du)
    B, D, seed, cb = gm.B, dc + du, 7 + C, 1000 * S + 3
    cands, err = gm.sample(C, seed, levels, counter_base=cb, requests=S)
    cands[5] = float("nan")  # a model, and no candidate with a score
    err[1, S - 1, C - 1] = 1  # what the sampler sets where truncnorm's bounds fail: that one request only
    if S == 1:  # the one-request form: hbx_kde_acquire_groups' records, pools [B, C, D]
        cands, err = cands.view(B, C, D), err.view(B, C)
        rec = gm.acquire(cands, sync=False)
    else:
        rec = gm.acquire_requests(cands, sync=False)
    before = rec.cpu().numpy().tobytes()
    r = _records(rec)
    ch, eh = cands.cpu().numpy().reshape(B * S, C, D), err.cpu().numpy().reshape(B * S, C)
    assert np.all(r["index"][5 * S:] == -1) and not np.any(r["flags"][5 * S:] & (NO_MODEL | UNSUPPORTED))
    seen = set()
    for rf in (0.0, 1.0 / 3, 1.0):
        out = gm.finish(cands, rec, err, levels, rf, seed, cb)
        want_rows, want_src = _restate(r, ch, eh, levels, C, rf, seed, cb, B * S)
        lead = (B,) if S == 1 else (B, S)
        assert out.rows.shape == lead + (D,) and out.source.shape == lead and out.source.dtype == np.uint8
        np.testing.assert_array_equal(out.source.reshape(-1), want_src)
        assert out.rows.tobytes() == want_rows.tobytes(), (rf, np.nonzero(out.rows.reshape(-1, D) != want_rows))
        np.testing.assert_array_equal(out.model_based, out.source == MODEL)
        seen |= set(int(v) for v in want_src)
        if rf == 0.0:
            assert {MODEL, SRC_NO_MODEL, NO_SCORE, DOMAIN_ERR} <= set(int(v) for v in want_src)
            assert want_src[1 * S + S - 1] == DOMAIN_ERR and np.all(want_src[5 * S:] == NO_SCORE)
            assert np.all(want_src[1 * S:1 * S + S - 1] == MODEL) and np.all(want_src[:S] == MODEL)
        if rf == 1.0:
            assert set(int(v) for v in want_src) == {RANDOM_FRACTION, SRC_NO_MODEL}
    assert seen == {MODEL, RANDOM_FRACTION, SRC_NO_MODEL, NO_SCORE, DOMAIN_ERR}
    assert rec.cpu().numpy().tobytes() == before  # the records are read, never written
    # no error bytes: the hand-set request is a model pick again; no records: every request a prior draw
    out = gm.finish(cands, rec, None, levels, 0.0, seed, cb)
    want_rows, want_src = _restate(r, ch, None, levels, C, 0.0, seed, cb, B * S)
    assert want_src[1 * S + S - 1] == MODEL
    assert out.source.tobytes() == want_src.tobytes() and out.rows.tobytes() == want_rows.tobytes()
    out = gm.finish(cands, None, err, levels, 0.0, seed, cb)
    want_rows, want_src = _restate(None, ch, eh, levels, C, 0.0, seed, cb, B * S)
    assert np.all(out.source == SRC_NO_MODEL)
    assert out.source.tobytes() == want_src.tobytes() and out.rows.tobytes() == want_rows.tobytes()


@pytest.mark.parametrize("C", [37, 64])
@pytest.mark.parametrize("dc,du", [(5, 2), (24, 8)])
def test_fused_equals_composition(device, dc, du, C):
    from hpbandster_amd import groups
    gm, X, seg, vt, levels, kinds = _six(device, dc, du)
    B, D, S, seed, cb, rf = gm.B, dc + du, 3, 11, 5000, 1.0 / 3
    fused = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, keep_pools=True)
    cands, err = gm.sample(C, seed, levels, counter_base=cb, requests=S)
    rec = gm.acquire_requests(cands, sync=False)
    comp = gm.finish(cands, rec, err, levels, rf, seed, cb)
    ch = cands.cpu().numpy()
    assert fused.cands.shape == (B, S, C, D) and fused.cands.tobytes() == ch.tobytes()
    assert fused.domain_err.shape == (B, S, C) and fused.domain_err.tobytes() == err.cpu().numpy().tobytes()
    picks = groups.GroupPicks.from_bytes(rec.cpu().numpy().tobytes(), B, S)
    for name in groups.GroupPicks.__slots__:
        assert getattr(fused.picks, name).tobytes() == getattr(picks, name).tobytes(), name
    assert fused.rows.shape == (B, S, D) and fused.rows.tobytes() == comp.rows.tobytes()
    assert fused.source.tobytes() == comp.source.tobytes()
    assert MODEL in fused.source and SRC_NO_MODEL in fused.source
    for b in range(B):  # the records are the oracle's picks
        for s in range(S):
            if kinds.get(b) in ("no_model", "unsupported"):
                assert picks.index[b, s] == -1 and fused.source[b, s] == SRC_NO_MODEL
                continue
            l, g = _oracle(gm, X, seg, vt, ch[:, s], b)
            want, scores = O.select(l, g)
            assert want >= 0 and picks.index[b, s] == want and picks.score[b, s] == scores[want]
            assert _same(picks.pdf_l[b, s], l[want]) and _same(picks.pdf_g[b, s], g[want])
            if fused.source[b, s] == MODEL:
                assert fused.rows[b, s].tobytes() == ch[b, s, want].tobytes()
    # without the optional outputs, and the one-request form
    bare = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, records=False)
    assert bare.picks is None and bare.cands is None and bare.rows.tobytes() == fused.rows.tobytes()
    one = gm.get_config(C, seed, levels, random_fraction=rf, counter_base=cb, keep_pools=True)
    c1, e1 = gm.sample(C, seed, levels, counter_base=cb)
    want = gm.finish(c1, gm.acquire(c1, sync=False), e1, levels, rf, seed, cb)
    assert one.rows.shape == (B, D) and one.source.shape == (B,) and one.picks.index.shape == (B,)
    assert one.cands.shape == (B, C, D) and one.cands.tobytes() == c1.cpu().numpy().tobytes()
    assert one.rows.tobytes() == want.rows.tobytes() and one.source.tobytes() == want.source.tobytes()


def test_a_group_does_not_see_the_others(device):
    from hpbandster_amd import groups
    dc, du, S, C, seed, cb, rf = 5, 2, 3, 37, 21, 777, 1.0 / 3
    D = dc + du
    rs = np.random.RandomState(5)
    levels = [0] * dc + [3] * du
    lens = np.array([40, D, 90, 64, 30])  # group 1: no model
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg[-1])
    X = np.hstack([rs.rand(n, dc), rs.randint(0, 3, (n, du)).astype(np.float64)])
    losses = rs.rand(n)
    vt = "c" * dc + "u" * du
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    np.testing.assert_array_equal(gm.has_model, [True, False, True, True, True])
    five = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, keep_pools=True)
    assert five.source[1].tolist() == [SRC_NO_MODEL] * S and MODEL in five.source
    for b in range(5):
        g1 = groups.fit_groups(X[seg[b]:seg[b + 1]], losses[seg[b]:seg[b + 1]], np.array([0, lens[b]], dtype=np.int64),
                               vt, device=device)
        one = g1.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb + b * S * C,
                            keep_pools=True)
        assert one.rows.tobytes() == five.rows[b].tobytes(), b
        assert one.source.tobytes() == five.source[b].tobytes(), b
        assert one.cands.tobytes() == five.cands[b].tobytes() and one.domain_err.tobytes() == five.domain_err[b].tobytes()
        for name in groups.GroupPicks.__slots__:
            if name not in ("shortlist", "near", "rel", "flags"):  # (the screen's diagnostics may depend on the launch)
                assert getattr(one.picks, name).tobytes() == getattr(five.picks, name)[b].tobytes(), (b, name)


@pytest.mark.parametrize("value,code", [(0.5, NO_SCORE), (0.0, DOMAIN_ERR)])
def test_real_failure_routes(device, value, code):
    """The good rows share one continuous value: bandwidth 0.  At 0.5 the draws succeed and every pdf is NaN (no
    score); at 0.0 truncnorm's bounds -m / h are NaN and every draw of that dim is a domain error."""
    from hpbandster_amd import groups
    dc, du, n, S, C, seed, cb, rf = 2, 1, 40, 8, 16, 3, 99, 1.0 / 3
    rs = np.random.RandomState(8)
    levels = [0, 0, 3]
    X = np.hstack([rs.rand(n, dc), rs.randint(0, 3, (n, du)).astype(np.float64)])
    losses = np.arange(n, dtype=np.float64)  # the good KDE: the head rows
    gm = groups.fit_groups(X, losses, np.array([0, n], dtype=np.int64), "ccu", device=device)
    X[:int(gm.n_good[0]), 0] = value
    gm = groups.fit_groups(X, losses, np.array([0, n], dtype=np.int64), "ccu", device=device)
    assert gm.has_model[0] and gm.bandwidths()[0][0, 0] == 0.0
    out = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, keep_pools=True)
    random = np.array([_decision(seed, cb + q * C) < rf for q in range(S)])
    assert not random.all()
    np.testing.assert_array_equal(out.source[0], np.where(random, RANDOM_FRACTION, code))
    assert bool(out.domain_err.any()) == (code == DOMAIN_ERR) and np.all(out.picks.index == -1)
    assert not out.model_based.any()
    for q in range(S):
        assert out.rows[0, q].tobytes() == _prior_row(levels, seed, cb + q * C).tobytes(), q


def test_prior_values(device):
    from hpbandster_amd import groups
    levels = [0, 0, 3, 0, 2, 0, 5]
    B, S, seed = 64, 64, 17
    out = groups.sample_prior(B, S, levels, seed, device=device)
    assert out.rows.shape == (B, S, 7) and np.all(out.source == SRC_NO_MODEL) and out.picks is None
    rows = out.rows.reshape(B * S, 7)
    for d, t in enumerate(levels):
        col = rows[:, d]
        if t == 0:
            assert np.all(col > 0.0) and np.all(col < 1.0)
        else:
            assert np.all(col == np.floor(col)) and np.all(col >= 0) and np.all(col < t)
            assert set(col.tolist()) == set(float(v) for v in range(t))  # 4096 draws: every level
    want = np.array([_prior_row(levels, seed, q) for q in range(B * S)])
    assert rows.tobytes() == want.tobytes()
    other = groups.sample_prior(B, S, levels, seed, counter_base=B * S, device=device)
    assert not set(r.tobytes() for r in rows) & set(r.tobytes() for r in other.rows.reshape(B * S, 7))
    # the counter stride C, a stream id, and the one-request form
    strided = groups.sample_prior(5, None, levels, seed, counter_base=10, C=16, stream_id=2, device=device)
    assert strided.rows.shape == (5, 7) and strided.source.shape == (5,)
    want = np.array([_prior_row(levels, seed, 10 + 16 * q, 2) for q in range(5)])
    assert strided.rows.tobytes() == want.tobytes()


def _loss(rows):
    return ((rows[..., 0] - 0.3) ** 2 + (rows[..., 1] - 0.7) ** 2 + 0.1 * rows[..., 2])


def test_group_bohb_end_to_end(device):
    """Three optimisers in lockstep equal three single ones fed the same results, round by round, across the
    no-model -> model boundary (n = 6 > min_points + 1 = 5 after the third round)."""
    from hpbandster_amd import groups
    B, S, C, budget = 3, 2, 16, 9.0
    kw = dict(var_type="ccu", levels=[0, 0, 4], num_samples=C, seed=42, device=device)
    opt = groups.GroupBOHB(B, **kw)
    singles = [groups.GroupBOHB(1, **kw) for _ in range(B)]
    modelled = []
    for t in range(6):
        cfg = opt.get_configs(budget, S=S)
        assert cfg.rows.shape == (B, S, 3) and cfg.source.shape == (B, S)
        assert opt.counter == (t + 1) * B * S * C
        for b in range(B):
            one = singles[b].get_configs(budget, S=S, counter_base=t * B * S * C + b * S * C)
            assert one.rows.tobytes() == cfg.rows[b].tobytes(), (t, b)
            assert one.source.tobytes() == cfg.source[b].tobytes(), (t, b)
        if not opt.kde_models:
            assert np.all(cfg.source == SRC_NO_MODEL)
        else:
            assert not np.any(cfg.source == SRC_NO_MODEL)
        modelled.append(bool(opt.kde_models))
        losses = _loss(cfg.rows)
        if t == 1:
            losses[2, 0] = np.inf  # a crashed run
        refit = opt.new_results(budget, cfg.rows, losses)
        assert refit == (2 * (t + 1) > 5)
        for b in range(B):
            singles[b].new_results(budget, cfg.rows[b:b + 1], losses[b:b + 1])
    assert modelled == [False, False, False, True, True, True]
    assert list(opt.kde_models) == [budget] and opt.kde_models[budget].B == B
    assert tuple(opt.configs[budget].shape) == (B, 12, 3)
    assert cfg.model_based.any()


def test_asynchronous_use(device):
    import torch
    gm, X, seg, vt, levels, kinds = _six(device, 5, 2)
    B, S, C, seed = gm.B, 3, 37, 31
    st = torch.cuda.Stream(device=device)
    a = gm.get_config(C, seed, levels, requests=S, counter_base=0, stream=st, sync=False)
    b = gm.get_config(C, seed, levels, requests=S, counter_base=B * S * C, stream=st, sync=False)  # queued behind a
    for out in (a, b):
        assert out.rows.is_cuda and out.source.is_cuda and out.model_based.is_cuda and out.picks.is_cuda
        assert tuple(out.rows.shape) == (B, S, 7) and tuple(out.picks.shape) == (B, S, 48)
    st.synchronize()
    for out, cb in ((a, 0), (b, B * S * C)):
        want = gm.get_config(C, seed, levels, requests=S, counter_base=cb, records=False)
        assert out.rows.cpu().numpy().tobytes() == want.rows.tobytes()
        assert out.source.cpu().numpy().tobytes() == want.source.tobytes()
    assert a.rows.cpu().numpy().tobytes() != b.rows.cpu().numpy().tobytes()
