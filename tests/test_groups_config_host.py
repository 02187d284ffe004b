"""Grouped get_config, host side (no GPU): the new entry points' signatures and argument handling, GroupConfigs'
shapes, and GroupBOHB's bookkeeping (bohb.py:198-217, :124) with the engine calls stubbed."""
import numpy as np
import pytest

NEW = ("hbx_kde_finish_groups", "hbx_kde_propose_groups_workspace_bytes", "hbx_kde_propose_groups_ws_offsets",
       "hbx_kde_propose_groups")


def test_new_symbols_have_signatures():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name in NEW:
        assert hasattr(L, name) and name in N.SIGNATURES, name
    assert len(N.SIGNATURES["hbx_kde_finish_groups"][1]) == 15
    assert len(N.SIGNATURES["hbx_kde_propose_groups"][1]) == 27


def test_finish_checks_its_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()

    def fin(rec=4096, cands=4096, err=4096, lv=4096, D=3, B=4, S=3, C=8, rf=0.25, rows=4096, src=4096):
        # non-null placeholders are never dereferenced: every check precedes the launch
        return L.hbx_kde_finish_groups(rec or None, cands or None, err or None, lv or None, D, B, S, C, rf, 1, 0, 0,
                                       rows or None, src or None, None)

    assert fin(lv=0) == -1 and b"hbx_kde_finish_groups" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert fin(rows=0) == -1 and fin(src=0) == -1
    assert fin(cands=0) == -1 and b"cands" in L.hbx_last_error()  # records without their pools
    assert fin(D=0) == -1 and fin(D=257) == -1
    assert fin(B=-1) == -1 and fin(S=-1) == -1 and b"S=-1" in L.hbx_last_error()
    assert fin(C=0) == -1 and fin(C=-2) == -1  # C >= 1: the counter stride
    assert fin(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert fin(rf=bad) == -1 and b"random_fraction" in L.hbx_last_error(), bad
    assert fin(rows=4100) == -1 and b"aligned" in L.hbx_last_error()
    assert fin(B=0) == 0 and fin(S=0) == 0  # nothing to do, nothing launched
    assert fin(B=0, lv=0, rows=0, src=0) == 0


def test_propose_checks_its_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()
    f = L.hbx_kde_propose_groups_workspace_bytes
    acq = L.hbx_kde_groups_batch_workspace_bytes
    B, S, C, D = 10, 4, 64, 32
    want = acq(B, S, C, D) + B * S * C * D * 8 + B * S * C + B * S * 48
    assert f(B, S, C, D) == want  # (every part a multiple of 16 at this shape)
    off = np.zeros(4, dtype=np.int64)
    assert L.hbx_kde_propose_groups_ws_offsets(B, S, C, D, off.ctypes.data) == 0
    assert list(off) == [acq(B, S, C, D), acq(B, S, C, D) + B * S * C * D * 8,
                         acq(B, S, C, D) + B * S * C * D * 8 + B * S * C, want]
    assert L.hbx_kde_propose_groups_ws_offsets(3, 1, 5, 3, off.ctypes.data) == 0
    assert np.all(off % 16 == 0) and np.all(np.diff(off) >= [3 * 5 * 3 * 8, 3 * 5, 3 * 48])
    assert f(0, 4, 64, 32) > 0 and f(10, 0, 64, 32) > 0  # zero-safe
    assert f(10, 4, 0, 32) == -1 and f(-1, 1, 1, 1) == -1 and f(1, 1, 1, 0) == -1 and f(1, 1, 1, 257) == -1
    assert f(1 << 12, 1 << 10, 1 << 10, 32) == -1
    assert L.hbx_kde_propose_groups_ws_offsets(B, S, C, D, None) == -1

    def prop(X=4096, lv=4096, D=3, B=4, S=3, C=8, rf=0.25, rows=4096, src=4096, ws=4096, wsb=1 << 30, rec=None,
             cands=None):
        p = 4096
        return L.hbx_kde_propose_groups(X or None, D, p, B, p, p, p, p, p, p, p, p, lv or None, 3.0, rf, 1, 0, 0, S,
                                        C, rows or None, src or None, rec, cands, ws or None, wsb, None)

    assert prop(X=0) == -1 and b"hbx_kde_propose_groups" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert prop(lv=0) == -1 and prop(rows=0) == -1 and prop(src=0) == -1 and prop(ws=0) == -1
    assert prop(D=0) == -1 and prop(D=257) == -1 and prop(B=-1) == -1 and prop(S=-1) == -1 and prop(C=0) == -1
    assert prop(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    for bad in (-0.5, 2.0, float("nan")):
        assert prop(rf=bad) == -1 and b"random_fraction" in L.hbx_last_error(), bad
    assert prop(wsb=f(4, 3, 8, 3) - 1) == -1 and b"workspace too small" in L.hbx_last_error()
    assert prop(ws=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert prop(rec=4100) == -1 and prop(cands=4100) == -1
    assert prop(B=0) == 0 and prop(S=0) == 0


def test_group_configs_shapes():
    from hpbandster_amd import groups
    B, S, D = 4, 3, 5
    rows = np.arange(B * S * D, dtype=np.float64).reshape(B * S, D)
    source = (np.arange(B * S) % 5).astype(np.uint8)
    c = groups.GroupConfigs(rows, source, B, S)
    assert len(c) == B and c.rows.shape == (B, S, D) and c.source.shape == (B, S) and c.source.dtype == np.uint8
    assert c.model_based.shape == (B, S) and c.model_based.dtype == bool
    np.testing.assert_array_equal(c.model_based, c.source == 0)
    np.testing.assert_array_equal(c.rows[2, 1], rows[2 * S + 1])  # request b * S + s is element [b, s]
    assert c.picks is None and c.cands is None and c.domain_err is None
    one = groups.GroupConfigs(rows[:B], source[:B], B)
    assert len(one) == B and one.rows.shape == (B, D) and one.source.shape == (B,) and one.model_based.shape == (B,)
    assert (groups.GroupConfigs.SOURCE_MODEL, groups.GroupConfigs.SOURCE_RANDOM_FRACTION,
            groups.GroupConfigs.SOURCE_NO_MODEL, groups.GroupConfigs.SOURCE_NO_SCORE,
            groups.GroupConfigs.SOURCE_DOMAIN_ERR) == (0, 1, 2, 3, 4)
    assert groups.SOURCE_DOMAIN_ERR == 4 and groups.SOURCE_NO_MODEL == 2
    empty = groups.GroupConfigs(np.empty((0, D)), np.empty(0, dtype=np.uint8), 0, S)
    assert len(empty) == 0 and empty.rows.shape == (0, S, D)
    assert "(4, 3)" in repr(c)
    with pytest.raises(ValueError):
        groups._fraction(1.5)
    with pytest.raises(ValueError):
        groups._fraction(float("nan"))


class _Model(object):
    """stands in for a GroupModel: records get_config's arguments"""

    def __init__(self, log, budget, n):
        self.log, self.budget, self.n = log, budget, n
        self.has_model = np.ones(2, dtype=bool)

    def get_config(self, C, seed, levels, **kw):
        self.log.append(("get_config", self.budget, C, seed, kw))
        return "model %r" % (self.budget,)


def _stubbed(monkeypatch, **kw):
    import torch
    from hpbandster_amd import groups
    log = []

    def fit_groups(X, losses, seg_off, var_type, min_points=None, top_n_percent=15, device=None, stream=None):
        n = int(seg_off[1])
        assert tuple(X.shape) == (2 * n, 3) and tuple(losses.shape) == (2 * n,)
        np.testing.assert_array_equal(seg_off, np.arange(3) * n)
        log.append(("fit", n, min_points, top_n_percent))
        return _Model(log, None, n)

    def sample_prior(B, S, levels, seed, counter_base=0, C=1, **k):
        log.append(("prior", B, S, seed, counter_base, C))
        return "prior"

    monkeypatch.setattr(groups, "fit_groups", fit_groups)
    monkeypatch.setattr(groups, "sample_prior", sample_prior)
    opt = groups.GroupBOHB(2, "ccu", [0, 0, 4], device=torch.device("cpu"), **kw)
    return opt, log


def _feed(opt, budget, m, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.rand(2, m, 3)
    X[:, :, 2] = rs.randint(0, 4, size=(2, m))
    return opt.new_results(budget, X, rs.rand(2, m)), X


def test_group_bohb_refits_first_at_min_points_plus_two(monkeypatch):
    opt, log = _stubbed(monkeypatch)
    assert opt.min_points_in_model == 4  # D + 1
    for n in range(1, 6):  # n <= min_points + 1 = 5: stored, no model (bohb.py:216-217)
        assert _feed(opt, 1.0, 1, seed=n)[0] is False
        assert tuple(opt.configs[1.0].shape) == (2, n, 3) and tuple(opt.losses[1.0].shape) == (2, n)
    assert log == [] and opt.kde_models == {}
    refit, X = _feed(opt, 1.0, 1, seed=9)
    assert refit is True and log == [("fit", 6, 4, 15)] and list(opt.kde_models) == [1.0]
    np.testing.assert_array_equal(opt.configs[1.0][:, -1].numpy(), X[:, 0])  # appended behind the earlier rows
    assert _feed(opt, 1.0, 3)[0] is True and log[-1] == ("fit", 9, 4, 15)  # m rows at once: one refit
    small = _stubbed(monkeypatch, min_points_in_model=2)[0]
    assert small.min_points_in_model == 4  # raised to D + 1 (bohb.py:55-57)
    big, blog = _stubbed(monkeypatch, min_points_in_model=7, top_n_percent=20)
    assert _feed(big, 3.0, 8)[0] is False and _feed(big, 3.0, 1)[0] is True and blog == [("fit", 9, 7, 20)]
    with pytest.raises(Exception):
        opt.new_results(1.0, np.zeros((3, 1, 3)), np.zeros((3, 1)))  # B is 2
    with pytest.raises(Exception):
        opt.new_results(1.0, np.zeros((2, 2, 3)), np.zeros((2, 1)))


def test_group_bohb_drops_a_smaller_budget_once_a_larger_model_exists(monkeypatch):
    opt, log = _stubbed(monkeypatch)
    _feed(opt, 1.0, 3)
    assert _feed(opt, 9.0, 6)[0] is True and list(opt.kde_models) == [9.0]
    n_before = len(log)
    assert _feed(opt, 1.0, 5)[0] is False  # bohb.py:204-205: not stored, not fit
    assert tuple(opt.configs[1.0].shape) == (2, 3, 3) and len(log) == n_before
    assert _feed(opt, 3.0, 6)[0] is False and tuple(opt.configs[3.0].shape) == (2, 0, 3)  # the key exists (:198-200)
    assert _feed(opt, 27.0, 6)[0] is True and sorted(opt.kde_models) == [9.0, 27.0]  # a larger budget is modelled
    assert _feed(opt, 9.0, 1)[0] is False and tuple(opt.configs[9.0].shape) == (2, 6, 3)
    inf = np.full((2, 1), np.inf)  # a crashed run: +inf is stored as it is (bohb.py:189-194)
    opt.new_results(27.0, np.zeros((2, 1, 3)), inf)
    assert np.isinf(opt.losses[27.0][:, -1].numpy()).all()


def test_group_bohb_largest_modelled_budget_answers_and_the_counter_advances(monkeypatch):
    opt, log = _stubbed(monkeypatch, num_samples=16, seed=5, random_fraction=0.25, bandwidth_factor=2)
    assert opt.get_configs(1.0, S=3) == "prior" and log[-1] == ("prior", 2, 3, 5, 0, 16)
    assert opt.counter == 2 * 3 * 16
    assert opt.get_configs(1.0) == "prior" and log[-1] == ("prior", 2, 1, 5, 96, 16) and opt.counter == 96 + 2 * 16
    assert opt.get_configs(1.0, S=2, counter_base=7) == "prior" and log[-1][4] == 7 and opt.counter == 128  # not moved
    _feed(opt, 1.0, 6)
    _feed(opt, 9.0, 7)
    opt.kde_models[1.0].budget, opt.kde_models[9.0].budget = 1.0, 9.0
    assert opt.get_configs(1.0, S=4) == "model 9.0"  # bohb.py:124: max(self.kde_models.keys()), whatever is asked
    name, budget, C, seed, kw = log[-1]
    assert (name, budget, C, seed) == ("get_config", 9.0, 16, 5)
    assert kw["requests"] == 4 and kw["counter_base"] == 128 and kw["random_fraction"] == 0.25
    assert kw["bandwidth_factor"] == 2 and kw["sync"] is True
    assert opt.counter == 128 + 2 * 4 * 16
    opt.get_configs(9.0, S=1, sync=False)
    assert log[-1][4]["counter_base"] == 256 and log[-1][4]["sync"] is False and opt.counter == 256 + 32
