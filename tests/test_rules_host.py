"""The acquisition rules (hbx_rules: pdf_floor, min_bandwidth) on the host side: the ABI table, the range checks in
Python and in C, the host re-score's formula, and the float the kernels take for ln f (no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RULES_FORMS = ("hbx_kde_fit_r", "hbx_kde_refit_r", "hbx_kde_refit_sync_r", "hbx_kde_pair_set_rules",
               "hbx_kde_acquire_groups_batch_r", "hbx_kde_acquire_groups_topk_r", "hbx_kde_propose_groups_r")


def test_rules_forms_in_the_abi_table():
    """Every rules-taking form is declared, exported and in the ctypes table: its plain form's arguments plus the
    rules pointer (the setter: handle and pointer); the plain forms keep their argument counts."""
    from hpbandster_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "hbx.h")).read()
    assert re.search(r"typedef struct \{\s*double pdf_floor;\s*double min_bandwidth;\s*\} hbx_rules;", hdr)
    L = N.lib()
    for name in RULES_FORMS:
        assert name in N.SIGNATURES and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
        if name.endswith("_r"):
            res, args = N.SIGNATURES[name]
            pres, pargs = N.SIGNATURES[name[:-2]]
            assert res == pres and args == pargs + [N.c_vp], name
    assert N.SIGNATURES["hbx_kde_pair_set_rules"] == (N.c_i32, [N.c_vp, N.c_vp])
    assert ctypes.sizeof(N.Rules) == 16 and N.Rules.pdf_floor.offset == 0 and N.Rules.min_bandwidth.offset == 8
    assert L.hbx_version().decode().startswith("hbx 0.3")


BAD_FLOORS = (0.0, -1e-8, 1e-101, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf"))
GOOD_FLOORS = (1e-100, 1e-32, 1e-8, 1e-3, 1.0)
BAD_MIN_BW = (-1e-300, -1.0, float("nan"), float("inf"), -float("inf"))
GOOD_MIN_BW = (None, 0.0, 1e-3, 5.0)


def test_ranges_in_python():
    from hpbandster_amd import _native as N
    from hpbandster_amd import configspace as CS
    from hpbandster_amd import groups, kde
    from hpbandster_amd.config_generators import BOHB
    for f in GOOD_FLOORS:
        assert N.check_pdf_floor(f) == f
    for m in GOOD_MIN_BW:
        assert N.check_min_bandwidth(m) == (0.0 if m is None else m)
    r = N.rules()
    assert (r.pdf_floor, r.min_bandwidth) == (1e-8, 0.0)
    space = CS.ConfigurationSpace(seed=1)
    space.add_hyperparameter(CS.UniformFloatHyperparameter("x", lower=0, upper=1))
    X, losses = np.random.RandomState(0).rand(20, 2), np.arange(20.0)
    for f in BAD_FLOORS:
        for call in (lambda: N.check_pdf_floor(f), lambda: N.rules(pdf_floor=f),
                     lambda: BOHB(space, pdf_floor=f), lambda: groups.GroupBOHB(2, "cc", [0, 0], pdf_floor=f),
                     lambda: kde.fit_pair(X, losses, "cc", 3, pdf_floor=f),
                     lambda: kde.ObservationStore(2, "cc", device="cpu").refit(3, pdf_floor=f),
                     lambda: kde.fit_pair_from_rows(X, [0, 1, 2], [3, 4, 5], "cc", [.1, .1], [.1, .1], [0, 0], [0, 0],
                                                    pdf_floor=f),
                     lambda: groups.fit_groups(X, losses, [0, 20], "cc", pdf_floor=f)):
            with pytest.raises(ValueError):
                call()
    for m in BAD_MIN_BW:
        for call in (lambda: N.check_min_bandwidth(m), lambda: N.rules(min_bandwidth=m),
                     lambda: BOHB(space, min_bandwidth=m), lambda: groups.GroupBOHB(2, "cc", [0, 0], min_bandwidth=m),
                     lambda: kde.fit_pair(X, losses, "cc", 3, min_bandwidth=m),
                     lambda: kde.ObservationStore(2, "cc", device="cpu").refit(3, min_bandwidth=m),
                     lambda: groups.fit_groups(X, losses, [0, 20], "cc", min_bandwidth=m)):
            with pytest.raises(ValueError):
                call()
    cg = BOHB(space, min_bandwidth=1e-3, pdf_floor=1e-32)
    assert (cg.min_bandwidth, cg.pdf_floor) == (1e-3, 1e-32)
    cg = BOHB(space)
    assert (cg.min_bandwidth, cg.pdf_floor) == (0.0, 1e-8)
    import torch
    opt = groups.GroupBOHB(2, "cc", [0, 0], min_bandwidth=None, pdf_floor=1e-8, device=torch.device("cpu"))
    assert (opt.min_bandwidth, opt.pdf_floor) == (0.0, 1e-8)


def test_ranges_in_c():
    """HBX_ERR_ARG from every rules-taking entry point, before anything else is looked at (host memory only)."""
    from hpbandster_amd import _native as N
    L = N.lib()
    h = L.hbx_kde_pair_bind(32, 1, 2, 3, 4, 0, 5, 6, 7, 8, 0, 24, 8, 10000)
    assert h
    buf = np.zeros(64)
    p = N.ptr(buf)

    def calls(r):
        a = ctypes.addressof(r)
        return {
            "hbx_kde_pair_set_rules": lambda: L.hbx_kde_pair_set_rules(h, a),
            "hbx_kde_fit": lambda: L.hbx_kde_fit_r(p, 2, p, 1, p, p, p, p, p, p, p, p, p, p, None, a),
            "hbx_kde_refit": lambda: L.hbx_kde_refit_r(p, p, 10, 2, p, p, 0, 3, 7, 0.5, 0.5, p, p, 1, p, p, 1, p, p, 0,
                                                       None, a),
            "hbx_kde_refit_sync": lambda: L.hbx_kde_refit_sync_r(p, p, 10, 2, p, p, 0, 3, 7, 0.5, 0.5, p, p, 1, p, p, 1,
                                                                 p, p, 0, None, p, a),
            "hbx_kde_acquire_groups_batch_r": lambda: L.hbx_kde_acquire_groups_batch_r(
                p, 2, p, 1, p, p, p, p, p, p, p, p, p, 1, 4, p, p, 1 << 20, None, a),
            "hbx_kde_acquire_groups_topk_r": lambda: L.hbx_kde_acquire_groups_topk_r(
                p, 2, p, 1, p, p, p, p, p, p, p, p, p, 4, 2, p, p, 1 << 20, None, a),
            "hbx_kde_propose_groups_r": lambda: L.hbx_kde_propose_groups_r(
                p, 2, p, 1, p, p, p, p, p, p, p, p, p, 3.0, 0.3, 1, 0, 0, 1, 4, p, p, p, p, p, 1 << 20, None, a),
        }

    try:
        for f in BAD_FLOORS:
            for name, call in calls(N.Rules(f, 0.0)).items():
                assert call() == -1, (name, f)
                msg = L.hbx_last_error()
                assert name.encode() in msg and b"pdf_floor" in msg, (name, f, msg)
        for m in BAD_MIN_BW:
            for name, call in calls(N.Rules(1e-8, m)).items():
                assert call() == -1, (name, m)
                assert b"min_bandwidth" in L.hbx_last_error(), (name, m)
        for f in GOOD_FLOORS:  # the handle takes every accepted floor, and NULL (the snapshot's rules)
            r = N.Rules(f, 1e-3)
            assert L.hbx_kde_pair_set_rules(h, ctypes.addressof(r)) == 0, f
        assert L.hbx_kde_pair_set_rules(h, None) == 0
        assert L.hbx_kde_pair_set_rules(None, None) == -1 and b"pair" in L.hbx_last_error()
    finally:
        L.hbx_kde_pair_free(h)


def test_host_score_under_a_floor():
    """exact_host.bohb_score against the formula (g > f ? g : f) / (f > l ? f : l), Python max() semantics."""
    from hpbandster_amd import exact_host as E
    nan, inf = float("nan"), float("inf")
    assert E.bohb_score(1e-9, 1e-9) == 1.0 and E.bohb_score(1e-9, 1e-9, 1e-8) == 1.0  # the default is the snapshot's
    vals = (0.0, 1e-120, 1e-100, 3e-33, 1e-32, 2e-9, 1e-8, 1e-3, 0.25, 1.0, 40.0, inf, nan)
    for f in GOOD_FLOORS:
        for l in vals:
            for g in vals:
                num = g if g > f else f
                den = f if f > l else l
                want = num / den
                got = E.bohb_score(l, g, f)
                assert (got != got and want != want) or got == want, (f, l, g, got, want)
        assert E.bohb_score(f / 2, f / 4, f) == 1.0  # both clamped: exactly f / f
        assert E.bohb_score(inf, 1.0, f) == 0.0 and math.isnan(E.bohb_score(nan, 1.0, f))
        assert E.bohb_score(0.5, nan, f) == f / (f if f > 0.5 else 0.5)  # a NaN g is the floor


def test_resolve_takes_the_floor():
    """exact_host.resolve under two floors picks differently where only the floor tells the candidates apart."""
    from hpbandster_amd import exact_host as E

    class K(object):
        def __init__(self, data):
            self.data, self.bw, self.var_type, self.nlev = data, np.array([0.05]), "c", [0]

    good, bad = K(np.array([[0.2], [0.21]])), K(np.array([[0.8], [0.81], [0.79]]))
    rows = np.array([[0.96], [0.68]])  # both l below 1e-8 and above 1e-100; the first has the smaller g
    idx = np.array([0, 1])
    l = [float(E.kde_pdf(good.data, good.bw, "c", [0], r)) for r in rows]
    g = [float(E.kde_pdf(bad.data, bad.bw, "c", [0], r)) for r in rows]
    assert 1e-100 < l[0] < l[1] < 1e-8 and 1e-8 < g[0] < g[1]
    a = E.resolve(good, bad, rows, idx)             # 1e-8: l clamped for both, the smaller g wins
    b = E.resolve(good, bad, rows, idx, 1e-100)     # 1e-100: l counts, the larger l wins
    assert a == (0, g[0] / 1e-8, l[0], g[0]) and b == (1, g[1] / l[1], l[1], g[1])


def test_ln_floor_as_float():
    """(float)log(1e-8) is (float)HBX_LN_CLAMP bit for bit, so a floor of 1e-8 named through the parameter gives the
    kernels the constant they have always compiled in; the margin max(1e-4, 2 ulp) is the default's 1e-4 over the
    whole accepted range and covers the rounding of ln f down to 1e-100."""
    src = open(os.path.join(ROOT, "hpbandster_amd", "csrc", "hbx_kde_impl.h")).read()
    m = re.search(r"#define HBX_LN_CLAMP \((-[0-9.]+)\)", src)
    assert m
    clamp = float(m.group(1))
    assert np.float32(math.log(1e-8)).tobytes() == np.float32(clamp).tobytes()
    assert np.float32(np.log(np.float64(1e-8))).tobytes() == np.float32(clamp).tobytes()
    assert "f == HBX_PDF_FLOOR_DEFAULT ? (float)HBX_LN_CLAMP : (float)log(f)" in src  # and the default never asks libm
    for f in (1e-8, 1e-100, 1.0, 1e-32):
        C = np.float32(math.log(f))
        ulp = np.nextafter(np.abs(C), np.float32(np.inf)) - np.abs(C)
        margin = max(np.float32(1e-4), np.float32(2) * ulp)
        assert margin == np.float32(1e-4), (f, margin)  # (2 ulp = 3.1e-5 at |C| = 230: 1e-4 holds over the range)
        assert margin >= 2 * abs(float(C) - math.log(f)), (f, margin)  # the rounding of ln f to float is covered
