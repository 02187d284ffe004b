"""Grouped successive halving, host side (no GPU): hbx_sh_advance_groups' signature and argument handling, and the
bookkeeping of GroupSuccessiveHalving / GroupHyperband -- ladders, call order, the k rule, the counter rule -- with
the engine calls (promotion, fills, compaction) stubbed."""
import numpy as np
import pytest


def test_symbol_and_signature():
    from hpbandster_amd import _native as N
    L = N.lib()
    assert hasattr(L, "hbx_sh_advance_groups") and len(N.SIGNATURES["hbx_sh_advance_groups"][1]) == 12


def test_advance_checks_its_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()

    def adv(rows=4096, D=3, seg=4096, B=4, mask=4096, fresh=4096, F=2, K=5, out=4096, src=4096, cnt=4096):
        # non-null placeholders are never dereferenced: every check precedes the launch
        return L.hbx_sh_advance_groups(rows or None, D, seg or None, B, mask or None, fresh or None, F, K, out or None,
                                       src or None, cnt or None, None)

    for bad in ("rows", "seg", "mask", "out", "src"):
        assert adv(**{bad: 0}) == -1, bad
        assert b"hbx_sh_advance_groups" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert adv(D=0) == -1 and adv(D=257) == -1 and b"D=257" in L.hbx_last_error()
    assert adv(B=-1) == -1 and adv(K=-1) == -1 and adv(F=-1) == -1 and b"F=-1" in L.hbx_last_error()
    assert adv(fresh=0, F=2) == -1 and b"fresh" in L.hbx_last_error()
    assert adv(rows=4100) == -1 and b"aligned" in L.hbx_last_error()
    assert adv(out=4100) == -1 and adv(fresh=4100) == -1 and adv(src=4098) == -1
    assert adv(B=0) == 0 and adv(K=0) == 0  # nothing to do, nothing launched
    assert adv(B=0, rows=0, seg=0, mask=0, out=0, src=0, cnt=0, fresh=0, F=0) == 0


class _Configs(object):
    def __init__(self, torch, B, S, D, tag):
        self.rows = torch.full((B, S, D), float(tag), dtype=torch.float64)
        self.model_based = torch.zeros((B, S), dtype=torch.bool)
        self.source = torch.full((B, S), 2, dtype=torch.uint8)


def _stubbed(monkeypatch, nadv_of, B=2, num_samples=16):
    """GroupBOHB on the CPU with new_results / get_configs recorded, the promotion and the compaction stubbed:
    ``nadv_of(k, n)`` gives the advancing counts [B] the promotion reports."""
    import torch
    from hpbandster_amd import groups, promote
    log = []
    opt = groups.GroupBOHB(B, "ccu", [0, 0, 4], num_samples=num_samples, device=torch.device("cpu"))

    def new_results(budget, X, losses):
        log.append(("new_results", budget, tuple(X.shape), opt.counter))

    def get_configs(budget, S=1, counter_base=None, sync=True):
        if counter_base is None:
            counter_base = opt.counter
            opt.counter += opt.B * S * opt.num_samples
        log.append(("get_configs", budget, S, counter_base, sync, opt.counter))
        return _Configs(torch, opt.B, S, 3, len(log))

    def promote_segments(loss, seg_off, k, device=None, stream=None, return_order=False, ties="numpy",
                         on_device=False):
        assert on_device and not return_order
        n = int(seg_off[1])
        np.testing.assert_array_equal(seg_off, np.arange(opt.B + 1) * n)
        assert tuple(loss.shape) == (opt.B * n,) and len(k) == opt.B
        log.append(("promote", n, float(k[0]), ties, opt.counter))
        nadv = torch.as_tensor(np.asarray(nadv_of(float(k[0]), n), dtype=np.int64))
        return torch.zeros(opt.B * n, dtype=torch.uint8), nadv

    def advance(rows, seg_off, mask, K, fresh=None, stream=None, sync=True, device=None, out=None):
        assert not sync and tuple(rows.shape)[1] == 3 and tuple(mask.shape) == (rows.shape[0],)
        log.append(("advance", int(rows.shape[0]) // opt.B, K, None if fresh is None else tuple(fresh.shape),
                    opt.counter))
        return (torch.zeros((opt.B, K, 3), dtype=torch.float64), torch.zeros((opt.B, K), dtype=torch.int32),
                torch.zeros((opt.B, 2), dtype=torch.int64))

    monkeypatch.setattr(opt, "new_results", new_results)
    monkeypatch.setattr(opt, "get_configs", get_configs)
    monkeypatch.setattr(promote, "promote_segments", promote_segments)
    monkeypatch.setattr(groups, "advance", advance)
    return opt, log


def _stage_inputs(B, n):
    import torch
    return torch.zeros((B, n, 3), dtype=torch.float64), torch.zeros((B, n), dtype=torch.float64)


def test_step_order_k_rule_and_counters_without_deficit(monkeypatch):
    from hpbandster_amd import groups
    opt, log = _stubbed(monkeypatch, lambda k, n: [int(k), int(k)])
    sh = groups.GroupSuccessiveHalving([9, 3, 1], [1.0, 3.0, 9.0])
    assert [sh.threshold(s) for s in (0, 1)] == [3, 1]
    opt.counter = 1000
    st = sh.step(opt, *_stage_inputs(2, 9), 0)
    # new_results first (the reference's new_result per job precedes process_results), then promote, then advance;
    # no fill call, yet its block of B * K * num_samples counters is reserved before the compaction
    assert [e[0] for e in log] == ["new_results", "promote", "advance"]
    assert log[0] == ("new_results", 1.0, (2, 9, 3), 1000)
    assert log[1] == ("promote", 9, 3.0, "numpy", 1000)
    assert log[2] == ("advance", 9, 3, None, 1000 + 2 * 3 * 16)
    assert opt.counter == 1000 + 2 * 3 * 16 and st.fills is None and st.counter_base == 1000
    assert tuple(st.rows.shape) == (2, 3, 3) and tuple(st.src.shape) == (2, 3) and tuple(st.counts.shape) == (2, 2)
    del log[:]
    sh.step(opt, *_stage_inputs(2, 3), 1)
    assert [e[0] for e in log] == ["new_results", "promote", "advance"] and log[1][1:3] == (3, 1.0)
    assert opt.counter == 1096 + 2 * 1 * 16
    del log[:]
    assert sh.step(opt, *_stage_inputs(2, 1), 2) is None  # the last stage: reported, never promoted
    assert log == [("new_results", 9.0, (2, 1, 3), 1128)] and opt.counter == 1128


def test_step_fills_when_a_run_has_a_deficit(monkeypatch):
    from hpbandster_amd import groups
    opt, log = _stubbed(monkeypatch, lambda k, n: [3, 2])  # run 1: one crashed run too many
    sh = groups.GroupSuccessiveHalving([9, 3, 1], [1.0, 3.0, 9.0], ties="stable")
    opt.counter = 64
    st = sh.step(opt, *_stage_inputs(2, 9), 0)
    assert [e[0] for e in log] == ["new_results", "promote", "get_configs", "advance"]
    assert log[1][3] == "stable"
    # the S = K request on the next budget, on the reserved block, without synchronising
    assert log[2] == ("get_configs", 3.0, 3, 64, False, 64 + 2 * 3 * 16)
    assert log[3] == ("advance", 9, 3, (2, 3, 3), 64 + 2 * 3 * 16)
    assert st.fills is not None and st.counter_base == 64 and opt.counter == 64 + 96


def test_resampling_k_rule(monkeypatch):
    from hpbandster_amd import groups
    opt, log = _stubbed(monkeypatch, lambda k, n: [int(np.ceil(k))] * 2)
    sh = groups.GroupSuccessiveHalving([9, 3, 1], [1.0, 3.0, 9.0], resampling_rate=0.5)
    assert sh.threshold(0) == 1.5 and sh.threshold(1) == 1  # max(min_samples_advance, n (1 - rate)), HB_iteration.py:242
    sh.step(opt, *_stage_inputs(2, 9), 0)
    assert log[1][:3] == ("promote", 9, 1.5)
    assert [e[0] for e in log] == ["new_results", "promote", "get_configs", "advance"]  # ceil(1.5) = 2 < 3: fills
    assert groups.GroupSuccessiveHalving([27, 9], [1, 3], resampling_rate=0.75, min_samples_advance=4).threshold(0) == 4


def test_argument_validation(monkeypatch):
    from hpbandster_amd import groups
    from hpbandster_amd import _native as N
    G = groups.GroupSuccessiveHalving
    with pytest.raises(ValueError):
        G([9, 3], [1.0, 3.0, 9.0])
    with pytest.raises(ValueError):
        G([], [])
    with pytest.raises(ValueError):
        G([3, 0], [1.0, 3.0])
    with pytest.raises(ValueError):
        G([3, 1], [1.0, 3.0], resampling_rate=1.5)
    with pytest.raises(ValueError):
        G([3, 1], [1.0, 3.0], ties="random")
    opt, log = _stubbed(monkeypatch, lambda k, n: [1, 1])
    sh = G([3, 1], [1.0, 3.0])
    with pytest.raises(ValueError):
        sh.step(opt, *_stage_inputs(2, 3), 2)
    with pytest.raises(N.HbxError):
        sh.step(opt, *_stage_inputs(2, 4), 0)  # the stage has 3 configurations
    with pytest.raises(N.HbxError):
        sh.step(opt, *_stage_inputs(3, 3), 0)  # B is 2
    assert log == []  # refused before anything is reported
    with pytest.raises(ValueError):
        groups.GroupHyperband(opt, eta=1)
    with pytest.raises(ValueError):
        groups.GroupHyperband(opt, min_budget=2, max_budget=1)
    with pytest.raises(ValueError):
        groups.GroupHyperband(opt, resampling_rate=-1)
    with pytest.raises(ValueError):
        groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9).run(1, lambda *a: None, keep="disk")


def test_hyperband_ladders_and_call_sequence(monkeypatch):
    import torch
    from hpbandster_amd import groups
    opt, log = _stubbed(monkeypatch, lambda k, n: [int(k), int(k)])
    hb = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=9)
    assert [hb.ladder(it) for it in range(4)] == [([9, 3, 1], [1.0, 3.0, 9.0]), ([3, 1], [3.0, 9.0]), ([3], [9.0]),
                                                  ([9, 3, 1], [1.0, 3.0, 9.0])]
    seen = []

    def objective(rows, budget, info):
        seen.append((info["iteration"], info["stage"], budget, tuple(rows.shape)))
        assert info["budget"] == budget
        return np.zeros(tuple(rows.shape)[:2])  # a host array is accepted

    res = hb.run(3, objective, keep="device")
    assert seen == [(0, 0, 1.0, (2, 9, 3)), (0, 1, 3.0, (2, 3, 3)), (0, 2, 9.0, (2, 1, 3)),
                    (1, 0, 3.0, (2, 3, 3)), (1, 1, 9.0, (2, 1, 3)), (2, 0, 9.0, (2, 3, 3))]
    names = [(e[0],) + tuple(e[1:3]) for e in log]
    assert names == [
        ("get_configs", 1.0, 9), ("new_results", 1.0, (2, 9, 3)), ("promote", 9, 3.0), ("advance", 9, 3),
        ("new_results", 3.0, (2, 3, 3)), ("promote", 3, 1.0), ("advance", 3, 1), ("new_results", 9.0, (2, 1, 3)),
        ("get_configs", 3.0, 3), ("new_results", 3.0, (2, 3, 3)), ("promote", 3, 1.0), ("advance", 3, 1),
        ("new_results", 9.0, (2, 1, 3)),
        ("get_configs", 9.0, 3), ("new_results", 9.0, (2, 3, 3))]
    # counters: S = ns[0] requests per iteration plus a block of B * K * num_samples per transition
    per = 2 * 16
    assert opt.counter == per * ((9 + 3 + 1) + (3 + 1) + 3)
    assert hb.iterations == 3 and len(res) == 6 and res[(1, 1)].budget == 9.0
    assert isinstance(res[(0, 0)].rows, torch.Tensor)
    np.testing.assert_array_equal(res[(0, 0)].src.numpy(), np.tile(-1 - np.arange(9), (2, 1)))
    assert hb.run(1, objective, keep=None).stages == [] and hb.iterations == 4 and seen[-1][0] == 3
