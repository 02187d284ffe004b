"""Grouped ln-pdf, the signed route's host side (no GPU): the flag at the C ABI and ``signed=`` in Python."""
import numpy as np
import pytest


def test_flag_bits_beyond_the_two_known_are_refused():
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    L = N.lib()
    p = 4096  # non-null placeholders are never dereferenced: every check precedes the first launch
    assert (groups.LOGPDF_FP64_ONLY, groups.LOGPDF_SIGNED, groups.GRP_SIGNED_L, groups.GRP_SIGNED_G) == (1, 4, 256, 512)
    for flags in (2, 8, 4 | 2, 4 | 8, 1 | 4 | 16, -1):
        for rc in (L.hbx_kde_logpdf_groups(p, 3, p, 4, p, p, p, p, p, p, p, p, p, 8, 1e-5, flags, p, p, p, p, 1 << 20, None),
                   L.hbx_kde_rank_logratio_groups(p, 3, p, 4, p, p, p, p, p, p, p, p, p, 8, 2, 1e-5, flags, p, p, 1 << 20,
                                                  None)):
            assert rc == -1 and b"hbx_kde_logpdf_groups: flags=" in L.hbx_last_error(), flags
    # the known bits pass the flag check (B == 0: nothing to do, nothing launched)
    for flags in (0, 1, 4, 5):
        assert L.hbx_kde_logpdf_groups(p, 3, p, 0, p, p, p, p, p, p, p, p, p, 8, 1e-5, flags, p, p, p, p, 1 << 20, None) == 0


@pytest.mark.parametrize("call", ["logpdf", "rank_logratio"])
def test_unknown_signed_route_is_refused(call):
    from hpbandster_amd import groups
    gm = groups.GroupModel(B=2, D=3, device=None)
    args = (np.zeros((2, 4, 3)),) + ((2,) if call == "rank_logratio" else ())
    with pytest.raises(ValueError, match="signed"):
        getattr(gm, call)(*args, signed="log")
