"""Grouped acquisition, host side (no GPU): the C ABI's argument handling and the per-group split sizes."""
import os

import numpy as np

from oracle import kde_oracle as O

NEW = ["hbx_kde_groups_workspace_bytes", "hbx_kde_acquire_groups", "hbx_kde_sample_groups"]


def test_symbols_exported_and_bound():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(N._HERE), "include", "hbx.h")).read()
    assert "#define HBX_ACQ_NO_MODEL    16" in hdr and "#define HBX_ACQ_UNSUPPORTED 32" in hdr


def test_workspace_bytes():
    from hpbandster_amd import _native as N
    f = N.lib().hbx_kde_groups_workspace_bytes
    assert f(1, 1, 1) > 0
    assert f(0, 64, 32) > 0 and f(10, 0, 32) > 0  # zero-safe
    prev = 0
    for B in (1, 2, 7, 1000, 10000):
        v = f(B, 64, 32)
        assert v > prev
        prev = v
    prev = 0
    for C in (1, 2, 64, 65, 300, 4096):
        v = f(100, C, 32)
        assert v > prev
        prev = v
    assert f(10000, 64, 32) >= 10000 * 64 * 16
    # bad arguments: negative sizes, D out of range, B * C past int32
    assert f(-1, 64, 32) < 0 and f(1, -1, 32) < 0 and f(1, 1, 0) < 0 and f(1, 1, 257) < 0
    assert f(1 << 20, 1 << 12, 32) < 0


def test_bad_arguments_are_errors():
    from hpbandster_amd import _native as N
    L = N.lib()

    def acq(B=4, C=8, D=3, X=1, res=1, ws=1, wsb=1 << 20):
        # non-null placeholders are never dereferenced: every check precedes the launch
        p = 4096
        return L.hbx_kde_acquire_groups(p if X else None, D, p, B, p, p, p, p, p, p, p, p, p, C, p if res else None,
                                        p if ws else None, wsb, None)

    assert acq(X=0) == -1 and b"hbx_kde_acquire_groups" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert acq(res=0) == -1
    assert acq(ws=0) == -1
    assert acq(B=-1) == -1 and b"B=-1" in L.hbx_last_error()
    assert acq(C=-3) == -1
    assert acq(D=0) == -1 and acq(D=257) == -1
    assert acq(B=1 << 20, C=1 << 12) == -1 and b"int32" in L.hbx_last_error()
    assert acq(wsb=16) == -1 and b"workspace too small" in L.hbx_last_error()
    assert acq(B=0) == 0  # nothing to do, nothing launched

    def smp(B=4, C=8, D=4, X=1, cands=4096):
        p = 4096
        return L.hbx_kde_sample_groups(p if X else None, D, p, B, p, p, p, p, 3.0, 1, 0, 0, C, cands, None, None)

    assert smp(X=0) == -1 and b"hbx_kde_sample_groups" in L.hbx_last_error()
    assert smp(cands=None) == -1
    assert smp(B=-2) == -1 and smp(C=-1) == -1 and smp(D=0) == -1
    assert smp(B=1 << 20, C=1 << 12) == -1 and b"int32" in L.hbx_last_error()
    assert smp(cands=4104) == -1 and b"aligned" in L.hbx_last_error()  # D even: 16-byte rows
    assert smp(B=0) == 0 and smp(C=0) == 0


def test_group_sizes_match_the_oracle_split():
    """Per-group (n_good, n_bad) on ragged segments against oracle.bohb_split's row counts; segments with rows <= D
    have no model.  (bohb_split also applies new_result's gate n <= min_points + 1, bohb.py:216-217, which is the
    caller's and not the refit's -- as for kde.fit_pair -- so those two sizes are compared against the size rule.)"""
    from hpbandster_amd import groups, kde
    rs = np.random.RandomState(5)
    for D, top in ((1, 15), (3, 15), (8, 33), (32, 15), (32, 50)):
        lens = np.array([0, 1, D - 1, D, D + 1, D + 2, D + 3, 2 * D + 5, 40, 100, 299, 1000, 1101])
        lens = lens[lens >= 0]
        ng, nb = groups.group_sizes(lens, D, None, top)
        assert ng.dtype == np.int64 and ng.shape == lens.shape
        for n, a, b in zip(lens, ng, nb):
            if n <= D:
                assert (a, b) == (0, 0), (D, n)
                continue
            if n > D + 2:
                sp = O.bohb_split(rs.rand(n, D), rs.rand(n), D + 1, top)
                want = (0, 0) if sp is None else (len(sp[0]), len(sp[1]))
            else:
                want = tuple(min(v, n) for v in O.bohb_split_sizes(n, D + 1, top))
            assert (a, b) == want, (D, n)
            assert kde.split_sizes(int(n), D, D + 1, top, "bohb") == ((a, b) if a else None)
    # an explicit min_points
    ng, nb = groups.group_sizes([50], 4, 20, 15)
    assert (ng[0], nb[0]) == (20, 42)
