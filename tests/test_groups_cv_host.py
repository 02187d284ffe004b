"""Grouped cv_ml bandwidths, host side (no GPU): the new symbols and the C ABI's argument handling."""
import os

import pytest

NEW = ["hbx_kde_cv_groups_workspace_bytes", "hbx_kde_cv_groups"]


def test_symbols_exported_and_bound():
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    L = N.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(N._HERE), "include", "hbx.h")).read()
    for name, value in (("EVAL", groups.CV_EVAL), ("ML", groups.CV_ML), ("CONVERGED", groups.CV_CONVERGED),
                        ("LIMIT", groups.CV_LIMIT), ("NOT_SEARCHABLE", groups.CV_NOT_SEARCHABLE),
                        ("NO_MODEL", groups.CV_NO_MODEL)):
        assert "#define HBX_CV_%s %d\n" % (name, value) in hdr


def test_bad_arguments_are_errors_before_any_launch():
    from hpbandster_amd import _native as N
    L = N.lib()
    wsb = L.hbx_kde_cv_groups_workspace_bytes
    assert wsb(0, 0, 1) > 0 and wsb(1000, 10, 32) >= 8000 and wsb(1000, 10, 33) < 0 and wsb(-1, 1, 4) < 0

    def cv(X=4096, D=4, B=3, mode=1, max_evals=1000, ws=4096, bytes_=1 << 20, bw=4096):
        p = 4096  # non-null placeholders are never dereferenced: every check precedes the launch
        return L.hbx_kde_cv_groups(X, 100, D, p, B, p, p, p, p, p, p, bw, p, mode, max_evals, p, p, p, ws, bytes_,
                                   None, None)

    assert cv(X=None) == -1 and b"hbx_kde_cv_groups" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert cv(ws=None) == -1 and cv(D=0) == -1 and cv(B=-1) == -1 and cv(mode=2) == -1 and cv(max_evals=0) == -1
    assert cv(D=33) == -3 and b"32" in L.hbx_last_error()
    assert cv(bw=4100) == -1 and b"misaligned" in L.hbx_last_error()
    assert cv(bytes_=16) == -1 and b"workspace too small" in L.hbx_last_error()
    assert cv(B=0) == 0  # nothing to do, nothing launched


def test_unknown_rule_is_refused():
    from hpbandster_amd import cv, groups
    with pytest.raises(ValueError):
        groups.GroupBOHB(2, "cc", [0, 0], bw_estimation="cv_ls")
    with pytest.raises(ValueError):
        cv.select_bandwidth([[0.0], [1.0]], "c", "cv_ls", search="device")
