"""The request mask of the grouped get_config calls (hbx_kde_sample_groups_m, hbx_kde_acquire_groups_batch_m,
hbx_kde_finish_groups_m, hbx_kde_propose_groups_m, hbx_kde_random_requests_groups) on the GPU.  One sentence is
checked, byte for byte: every wanted request gets exactly what the dense call gives it, and an unwanted request is
not computed and is marked as skipped.  The dense calls are the reference; nothing here has a tolerance."""
import numpy as np
import pytest

from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

NO_MODEL, UNSUPPORTED, OVERFLOW, SKIPPED = 16, 32, 1, 64
SRC_RANDOM, SRC_SKIPPED = 1, 5
DECIDE_WORD = 0xFFFFFFFE
PATTERN = 0xA5
SHAPES = [(5, 8), (4, 64), (5, 40)]  # one straddling tile; tile = request; four straddling tiles
SEED, CB = 11, 4096

_MODELS = {}


def _model(device, name):
    """(a) B = 6, 2c + 1u (3 levels), 24 rows per group -- group 2 has 3 rows (no model: the reference wants
    more rows than dims, bohb.py:234-237, so D = 3 rows is the largest group without one), group 4's categorical
    column is constant (one observed level: exact-only); (b) B = 3, 24c + 8u (4 levels), 240 rows per group
    (n_good = 36, n_bad = 204: the fast piece counts).  (gm, levels, screenable groups)"""
    from hpbandster_amd import groups
    if name not in _MODELS:
        rs = np.random.RandomState(5 if name == "a" else 6)
        if name == "a":
            dc, du, nl, lens = 2, 1, 3, np.array([24, 24, 3, 24, 24, 24])
        else:
            dc, du, nl, lens = 24, 8, 4, np.array([240, 240, 240])
        seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(seg[-1])
        X = np.concatenate((rs.rand(n, dc), rs.randint(0, nl, size=(n, du)).astype(np.float64)), axis=1)
        if name == "a":
            X[seg[4]:seg[5], dc] = 1.0
        gm = groups.fit_groups(X, rs.rand(n), seg, "c" * dc + "u" * du, device=device)
        levels = [0] * dc + [nl] * du
        if name == "a":
            np.testing.assert_array_equal(gm.has_model, [True, True, False, True, True, True])
            screenable = [0, 1, 3, 5]
        else:
            assert np.all(gm.has_model) and int(gm.n_good[0]) == 36 and int(gm.n_bad[0]) == 204
            screenable = [0, 1, 2]
        _MODELS[name] = (gm, levels, screenable)
    return _MODELS[name]


def _masks(B, S):
    """name -> what the caller passes (a mask [B, S], or counts [B]) and the mask it means"""
    rs = np.random.RandomState(100 * B + S)
    bern = (rs.rand(B, S) < 0.5).astype(np.uint8)
    bern[0], bern[B - 1] = 0, 1
    counts = np.array(([0, S, 1] + [2, S - 1, 3])[:B], dtype=np.int64)
    return {"ones": (np.ones((B, S), np.uint8),) * 2, "zeros": (np.zeros((B, S), np.uint8),) * 2,
            "bernoulli": (bern,) * 2, "counts": (counts, (np.arange(S)[None, :] < counts[:, None]).astype(np.uint8))}


def _rec(t):
    from hpbandster_amd import groups
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=groups.RECORD)


def _raw(t, Q):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=np.uint8).reshape(Q, -1)


_DENSE = {}


def _dense(device, name, S, C, screen):
    """the dense calls' outputs, computed once per (model, shape, screen) and left unchanged"""
    key = (name, S, C, screen)
    if key not in _DENSE:
        gm, levels, _ = _model(device, name)
        pool, err = gm.sample(C, SEED, levels, counter_base=CB, requests=S)
        rec = gm.acquire_requests(pool, sync=False)
        fin = gm.finish(pool, rec, err, levels, 1.0 / 3, SEED, CB)
        cfg = gm.get_config(C, SEED, levels, requests=S, counter_base=CB, keep_pools=True)
        _DENSE[key] = dict(pool=pool.cpu().numpy(), err=err.cpu().numpy(), rec=_raw(rec, gm.B * S), fin=fin, cfg=cfg)
    return _DENSE[key]


def _check_skipped_records(raw, m, dense_raw):
    from hpbandster_amd import groups
    r, d = raw.view(groups.RECORD).reshape(-1), dense_raw.view(groups.RECORD).reshape(-1)
    off = m.reshape(-1) == 0
    assert np.all(r["index"][off] == -1) and np.all(r["shortlist"][off] == 0) and np.all(r["near"][off] == 0)
    assert np.all(np.isnan(r["score"][off])) and np.all(np.isnan(r["pdf_l"][off])) and np.all(np.isnan(r["pdf_g"][off]))
    np.testing.assert_array_equal(r["flags"][off], SKIPPED | (d["flags"][off] & (NO_MODEL | UNSUPPORTED)))
    assert not np.any(r["flags"][~off] & SKIPPED)


@pytest.mark.parametrize("screen", [0, 1, 2])
@pytest.mark.parametrize("S,C", SHAPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_wanted_requests_get_the_dense_bytes(device, monkeypatch, name, S, C, screen):
    import torch
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    if screen:
        monkeypatch.setenv("HBX_GROUPS_SCREEN", str(screen))
    else:
        monkeypatch.delenv("HBX_GROUPS_SCREEN", raising=False)
    gm, levels, screenable = _model(device, name)
    B, D, Q = gm.B, gm.D, gm.B * S
    dn = _dense(device, name, S, C, screen)
    if name == "a":  # the kinds the mask has to carry: no model; exact-only (re-scored whole)
        fl = dn["rec"].view(groups.RECORD).reshape(B, S)["flags"]
        assert np.all(fl[2] & NO_MODEL) and np.all(fl[4] & OVERFLOW) and not np.any(fl[4] & (NO_MODEL | UNSUPPORTED))
    lvd = torch.tensor(levels, dtype=torch.int32, device=device)
    for mname, (given, m) in _masks(B, S).items():
        tag = "%s %s" % (mname, (name, S, C, screen))
        on = m.reshape(-1) != 0
        md = torch.from_numpy(m).to(device)
        # ---- the sampler, into a buffer that holds a byte pattern
        pool = torch.full((B, S, C, D), 0, dtype=torch.float64, device=device)
        pool.view(torch.uint8).fill_(PATTERN)
        err = torch.full((B, S, C), 7, dtype=torch.uint8, device=device)
        N.check(N.lib().hbx_kde_sample_groups_m(*(gm.model_args(groups.SAMPLE_ARGS) + (
            N.ptr(lvd), 3.0, SEED, CB, 0, S, C, N.ptr(md), N.ptr(pool), N.ptr(err), N.stream_handle(None, device)))))
        ph = pool.cpu().numpy().reshape(Q, C * D)
        assert ph[on].tobytes() == dn["pool"].reshape(Q, C * D)[on].tobytes(), tag
        assert np.all(ph[~on].view(np.uint8) == PATTERN), tag
        eh = err.cpu().numpy().reshape(Q, C)
        np.testing.assert_array_equal(eh[on], dn["err"].reshape(Q, C)[on], err_msg=tag)
        assert not eh[~on].any(), tag
        p2, e2 = gm.sample(C, SEED, levels, counter_base=CB, requests=S, want=given)
        assert p2.cpu().numpy().reshape(Q, C * D)[on].tobytes() == ph[on].tobytes(), tag
        # ---- the acquisition over that pool (the unwanted requests' rows are the pattern: never read)
        ws = torch.empty(gm.workspace_bytes(C, S), dtype=torch.uint8, device=device)
        rec = gm.acquire_requests(pool, sync=False, workspace=ws, want=given)
        raw = _raw(rec, Q)
        assert raw[on].tobytes() == dn["rec"][on].tobytes(), (tag, np.nonzero((raw != dn["rec"]).any(axis=1) & on))
        _check_skipped_records(raw, m, dn["rec"])
        st = gm.request_stats(ws)
        assert st[0] == int(on.sum()) and st[0] + st[1] == Q, (tag, st)
        assert st[2] == C * int(m[screenable].sum()), (tag, st)  # skipped requests were not scored
        assert st[3] == int(raw.view(groups.RECORD).reshape(-1)["shortlist"].sum()), (tag, st)
        # ---- the finish step
        fin = gm.finish(pool, rec, err, levels, 1.0 / 3, SEED, CB, want=given)
        fr, fs = fin.rows.reshape(Q, D), fin.source.reshape(Q)
        assert fr[on].tobytes() == dn["fin"].rows.reshape(Q, D)[on].tobytes(), tag
        np.testing.assert_array_equal(fs[on], dn["fin"].source.reshape(Q)[on], err_msg=tag)
        assert np.all(fs[~on] == SRC_SKIPPED) and np.all(np.isnan(fr[~on])), tag
        assert not fin.model_based.reshape(Q)[~on].any()
        # ---- the fused call
        cfg = gm.get_config(C, SEED, levels, requests=S, counter_base=CB, keep_pools=True, want=given)
        dc = dn["cfg"]
        cr, cs = cfg.rows.reshape(Q, D), cfg.source.reshape(Q)
        assert cr[on].tobytes() == dc.rows.reshape(Q, D)[on].tobytes(), tag
        np.testing.assert_array_equal(cs[on], dc.source.reshape(Q)[on], err_msg=tag)
        assert np.all(cs[~on] == SRC_SKIPPED) and np.all(np.isnan(cr[~on])), tag
        assert cfg.cands.reshape(Q, C * D)[on].tobytes() == dc.cands.reshape(Q, C * D)[on].tobytes(), tag
        assert np.all(np.isnan(cfg.cands.reshape(Q, C * D)[~on])), tag
        np.testing.assert_array_equal(cfg.domain_err.reshape(Q, C)[on], dc.domain_err.reshape(Q, C)[on])
        for f in groups.GroupPicks.__slots__:
            a, b = getattr(cfg.picks, f).reshape(Q), getattr(dc.picks, f).reshape(Q)
            assert a[on].tobytes() == b[on].tobytes(), (tag, f)
        assert np.all(cfg.picks.flags.reshape(Q)[~on] & SKIPPED)
        if mname == "ones":  # the all-ones mask equals the dense call on every output, whole
            assert ph.tobytes() == dn["pool"].tobytes() and raw.tobytes() == dn["rec"].tobytes()
            assert fr.tobytes() == dn["fin"].rows.tobytes() and cr.tobytes() == dc.rows.tobytes()
            assert cfg.cands.tobytes() == dc.cands.tobytes() and cfg.domain_err.tobytes() == dc.domain_err.tobytes()


@pytest.mark.parametrize("S,C", SHAPES)
def test_want_none_is_the_dense_call(device, S, C):
    """want == NULL through every _m entry point: the dense outputs, whole (and every request counted as answered)"""
    import torch
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    gm, levels, screenable = _model(device, "a")
    B, D, Q = gm.B, gm.D, gm.B * S
    dn = _dense(device, "a", S, C, 0)
    lvd = torch.tensor(levels, dtype=torch.int32, device=device)
    sh = N.stream_handle(None, device)
    pool = torch.empty((B, S, C, D), dtype=torch.float64, device=device)
    err = torch.empty((B, S, C), dtype=torch.uint8, device=device)
    N.check(N.lib().hbx_kde_sample_groups_m(*(gm.model_args(groups.SAMPLE_ARGS) + (
        N.ptr(lvd), 3.0, SEED, CB, 0, S, C, None, N.ptr(pool), N.ptr(err), sh))))
    assert pool.cpu().numpy().tobytes() == dn["pool"].tobytes() and err.cpu().numpy().tobytes() == dn["err"].tobytes()
    ws = torch.empty(gm.workspace_bytes(C, S), dtype=torch.uint8, device=device)
    rec = torch.empty((Q, 48), dtype=torch.uint8, device=device)
    N.check(N.lib().hbx_kde_acquire_groups_batch_m(*(gm.model_args() + (
        N.ptr(pool), S, C, None, N.ptr(rec), N.ptr(ws), ws.numel(), sh, None))))
    assert _raw(rec, Q).tobytes() == dn["rec"].tobytes()
    st = gm.request_stats(ws)
    assert st[0] == Q and st[1] == 0 and st[2] == C * S * len(screenable)
    rows = torch.empty((Q, D), dtype=torch.float64, device=device)
    src = torch.empty(Q, dtype=torch.uint8, device=device)
    N.check(N.lib().hbx_kde_finish_groups_m(N.ptr(rec), N.ptr(pool), N.ptr(err), N.ptr(lvd), D, B, S, C, 1.0 / 3, SEED,
                                            CB, 0, None, N.ptr(rows), N.ptr(src), sh))
    assert rows.cpu().numpy().tobytes() == dn["fin"].rows.tobytes()
    assert src.cpu().numpy().tobytes() == dn["fin"].source.tobytes()


def _host_random_mask(B, S, C, rf, want_in=None):
    ctrs = [CB + q * C for q in range(B * S)]
    r = R.blocks(SEED, ctrs, DECIDE_WORD, 0)
    u = np.array([(float(((int(a) << 32) | int(b)) >> 11) + 0.5) * 2.0 ** -53 for a, b in zip(r[:, 0], r[:, 1])])
    m = ~(u < rf)
    if want_in is not None:
        m &= want_in.reshape(-1) != 0
    return m.astype(np.uint8).reshape(B, S)


@pytest.mark.parametrize("rf", [0.0, 1.0 / 3, 1.0])
@pytest.mark.parametrize("S,C", SHAPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_skip_random(device, name, S, C, rf):
    import torch
    from hpbandster_amd import _native as N
    gm, levels, screenable = _model(device, name)
    B, Q = gm.B, gm.B * S
    # the mask itself, against the host's Philox
    given, m = _masks(B, S)["bernoulli"]
    for want_in in (None, m):
        out = torch.full((B, S), 9, dtype=torch.uint8, device=device)
        wd = None if want_in is None else torch.from_numpy(want_in).to(device)
        N.check(N.lib().hbx_kde_random_requests_groups(B, S, C, rf, SEED, CB, 0, N.ptr(wd), N.ptr(out),
                                                       N.stream_handle(None, device)))
        np.testing.assert_array_equal(out.cpu().numpy(), _host_random_mask(B, S, C, rf, want_in))
    # the fused call: rows and sources of the plain call at every position, skipped records where source == 1
    plain = gm.get_config(C, SEED, levels, requests=S, random_fraction=rf, counter_base=CB)
    ws = torch.empty(gm.workspace_bytes_get_config(C, S, masked=True), dtype=torch.uint8, device=device)
    skip = gm.get_config(C, SEED, levels, requests=S, random_fraction=rf, counter_base=CB, skip_random=True,
                         workspace=ws, keep_pools=True)
    assert skip.rows.tobytes() == plain.rows.tobytes()
    assert skip.source.tobytes() == plain.source.tobytes()
    rnd = plain.source == SRC_RANDOM
    eff = _host_random_mask(B, S, C, rf)
    sk = (skip.picks.flags & SKIPPED) != 0
    np.testing.assert_array_equal(sk, eff == 0)  # the records follow the mask the sampler and the screens ran under
    hm = gm.has_model  # ... which, in groups that have a model, is exactly where the source is the random fraction
    np.testing.assert_array_equal(sk[hm], rnd[hm])
    assert not rnd[~hm].any() and np.all(skip.picks.flags[~hm] & NO_MODEL)  # (rule 2 first: the group's bit survives)
    if rf == 1.0 and name == "b":
        assert rnd.all()
    for f in skip.picks.__slots__:  # every other record is the plain call's
        assert getattr(skip.picks, f)[~sk].tobytes() == getattr(plain.picks, f)[~sk].tobytes(), f
    assert np.all(np.isnan(skip.cands[rnd]))  # a random request's pool is not written
    st = gm.request_stats(ws)
    assert st[0] + st[1] == Q and st[1] == int((eff == 0).sum())
    assert st[2] == C * int(eff[screenable].sum())
    # ... and under a mask as well: the skipped sources stay, the random ones among the wanted are not scored
    both = gm.get_config(C, SEED, levels, requests=S, random_fraction=rf, counter_base=CB, skip_random=True,
                         want=given, workspace=ws)
    on = m != 0
    assert both.rows[on].tobytes() == plain.rows[on].tobytes() and np.all(both.source[~on] == SRC_SKIPPED)
    assert gm.request_stats(ws)[2] == C * int((eff & m)[screenable].sum())


# ---- successive halving: fills="needed" ---------------------------------------------------------------------------
KW = dict(var_type="ccu", levels=[0, 0, 4], num_samples=16, seed=6)


def _loss(rows):
    return (rows[..., 0] - 0.3) ** 2 + (rows[..., 1] - 0.7) ** 2 + 0.1 * rows[..., 2]


def test_step_fills_needed_equals_all(device):
    """B = 4, ladder [9, 3, 1]; run 1 keeps two finite losses and run 2 none: deficits [0, 1, 3, 0]"""
    import torch
    from hpbandster_amd import groups
    out = {}
    for fills in ("all", "needed"):
        opt = groups.GroupBOHB(4, device=device, **KW)
        sh = groups.GroupSuccessiveHalving([9, 3, 1], [1.0, 3.0, 9.0], fills=fills)
        rows = opt.get_configs(1.0, S=9, sync=False).rows
        losses = _loss(rows.cpu().numpy())
        losses[1, 2:] = np.inf
        losses[2, :] = np.inf
        nxt = sh.step(opt, rows, torch.from_numpy(losses).to(device), 0)
        assert 1.0 in opt.kde_models  # the fills come from a model
        out[fills] = (nxt, opt.counter)
    a, n = out["all"][0], out["needed"][0]
    np.testing.assert_array_equal(a.counts.cpu().numpy()[:, 1], [0, 1, 3, 0])
    for f in ("rows", "src", "counts"):
        assert getattr(a, f).cpu().numpy().tobytes() == getattr(n, f).cpu().numpy().tobytes(), f
    assert out["all"][1] == out["needed"][1] and a.counter_base == n.counter_base
    src = n.fills.source.cpu().numpy()
    need = (np.arange(3)[None, :] < np.array([0, 1, 3, 0])[:, None])
    assert np.all(src[~need] == SRC_SKIPPED) and not np.any(src[need] == SRC_SKIPPED)
    assert n.fills.rows.cpu().numpy()[need].tobytes() == a.fills.rows.cpu().numpy()[need].tobytes()


def test_hyperband_fills_needed_equals_all(device):
    from hpbandster_amd import groups

    def objective(rows, budget, info):
        r = rows.cpu().numpy()
        out = _loss(r) / budget
        if budget == 1.0:
            out[1, r[1, :, 0] > 0.5] = np.inf  # run 1 comes out short
        return out

    res = {}
    for fills in ("all", "needed"):
        opt = groups.GroupBOHB(3, device=device, **KW)
        res[fills] = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9, fills=fills).run(2, objective)
    a, n = res["all"], res["needed"]
    assert len(a) == len(n) and len(a) > 0
    for ra, rn in zip(a.stages, n.stages):
        assert (ra.iteration, ra.stage, ra.budget) == (rn.iteration, rn.stage, rn.budget)
        for f in ("rows", "losses", "src", "model_based"):
            assert getattr(ra, f).tobytes() == getattr(rn, f).tobytes(), (ra.iteration, ra.stage, f)
    for x, y in zip(a.incumbent(), n.incumbent()):
        assert x.tobytes() == y.tobytes()


def test_get_configs_counts_with_conditions(device):
    """dim 1 is active when dim 2 is level 0 or 1: inactive dims NaN at wanted rows, skipped rows NaN whole -- on
    the prior path and on the model's"""
    from hpbandster_amd import groups
    opt = groups.GroupBOHB(3, device=device, impute_seed=3, conditions=[(1, 2, [0, 1])], **KW)
    counts = np.array([0, 4, 1])
    need = np.arange(4)[None, :] < counts[:, None]
    for path in ("prior", "model"):
        dense = opt.get_configs(1.0, S=4, counter_base=5000)
        part = opt.get_configs(1.0, S=4, counter_base=5000, counts=counts)
        assert part.rows[need].tobytes() == dense.rows[need].tobytes(), path
        np.testing.assert_array_equal(part.source[need], dense.source[need])
        assert np.all(part.source[~need] == SRC_SKIPPED) and np.all(np.isnan(part.rows[~need])), path
        w = part.rows[need]
        np.testing.assert_array_equal(np.isnan(w[:, 1]), w[:, 2] >= 2)
        assert not np.isnan(w[:, [0, 2]]).any()
        assert not part.model_based[~need].any()
        if path == "prior":
            first = opt.get_configs(1.0, S=12)
            assert opt.new_results(1.0, first.rows, _loss(np.nan_to_num(first.rows, nan=0.5)))


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(device):
    import torch
    from hpbandster_amd import _native as N
    gm, levels, _ = _model(device, "a")
    B, S, C = gm.B, 5, 8
    given, m = _masks(B, S)["bernoulli"]
    good = torch.from_numpy(m).to(device)
    pool, err = gm.sample(C, SEED, levels, counter_base=CB, requests=S)

    def one(k, w, ws=None):
        if k == 0:
            return gm.get_config(C, SEED, levels, requests=S, counter_base=CB, want=w, workspace=ws)
        if k == 1:
            return gm.acquire_requests(pool, want=w)
        if k == 2:
            return gm.finish(pool, None, None, levels, seed=SEED, want=w)
        return gm.sample(C, SEED, levels, counter_base=CB, requests=S, want=w)

    def calls(w, ws=None):
        return tuple(one(k, w, ws) for k in range(4))

    before = calls(good)
    wide = torch.ones((B, 2 * S), dtype=torch.uint8, device=device)
    bad = {"float": good.double(), "S + 1": torch.ones((B, S + 1), dtype=torch.uint8, device=device),
           "non-contiguous": wide[:, ::2], "host tensor": good.cpu(), "float array": m.astype(np.float64),
           "counts B + 1": np.ones(B + 1, dtype=np.int64), "int32 mask": good.int()}
    assert not bad["non-contiguous"].is_contiguous() and bad["non-contiguous"].shape == good.shape
    for what, w in bad.items():
        for k in range(4):
            with pytest.raises(N.HbxError):
                one(k, w)
                pytest.fail("call %d took a mask with %s" % (k, what))
    wsb = gm.workspace_bytes_get_config(C, S, masked=True)
    assert wsb > gm.workspace_bytes_get_config(C, S)
    with pytest.raises(N.HbxError, match="workspace too small"):
        gm.get_config(C, SEED, levels, requests=S, counter_base=CB, want=good,
                      workspace=torch.empty(wsb - 1, dtype=torch.uint8, device=device))
    with pytest.raises(N.HbxError, match="workspace too small"):
        gm.acquire_requests(pool, want=good,
                            workspace=torch.empty(gm.workspace_bytes(C, S) - 1, dtype=torch.uint8, device=device))
    after = calls(good, torch.empty(wsb, dtype=torch.uint8, device=device))  # exactly the helper's size is enough
    on = m != 0
    assert after[0].rows.tobytes() == before[0].rows.tobytes() and after[0].source.tobytes() == before[0].source.tobytes()
    for f in before[1].__slots__:
        assert getattr(after[1], f).tobytes() == getattr(before[1], f).tobytes(), f
    assert after[2].rows.tobytes() == before[2].rows.tobytes()
    assert after[3][0].cpu().numpy()[on].tobytes() == before[3][0].cpu().numpy()[on].tobytes()
