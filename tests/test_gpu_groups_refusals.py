"""What the five grouped calls that take a caller's pool refuse (GroupModel.acquire, acquire_requests, acquire_topk,
logpdf, finish): a device tensor of another dtype or not contiguous, a wrong leading B, trailing D or rank and, where
the call takes one, a workspace one byte short -- each an N.HbxError, and none leaves anything behind: the well-formed
call after the refusals answers what it answered before them, array for array.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, DC, LEVELS, N_ROWS, C, S, K = 3, 2, 3, 12, 8, 2, 3
D = DC + 1
METHODS = ["acquire", "acquire_requests", "acquire_topk", "logpdf", "finish"]


@pytest.fixture(scope="module")
def model(device):
    """(gm, levels, pool [B, S, C, D], domain_err [B, S, C], records of acquire_requests over the pool)"""
    from hpbandster_amd import groups
    rs = np.random.RandomState(11)
    X = np.concatenate((rs.rand(B * N_ROWS, DC), rs.randint(0, LEVELS, size=(B * N_ROWS, 1))), axis=1)
    losses = rs.rand(B * N_ROWS)
    seg = np.arange(B + 1, dtype=np.int64) * N_ROWS
    gm = groups.fit_groups(X, losses, seg, "c" * DC + "u", device=device)
    assert np.all(gm.has_model)
    levels = [0] * DC + [LEVELS]
    pool, err = gm.sample(C, 5, levels, requests=S)
    return gm, levels, pool, err, gm.acquire_requests(pool, sync=False)


def _arrays(r):
    """every slot of a result object that holds something, as host arrays by name"""
    return {name: np.asarray(getattr(r, name)) for name in r.__slots__ if getattr(r, name) is not None}


def _case(model, method):
    """(call(cands, workspace), the well-formed pool, the wrong-rank pool, workspace bytes or None)"""
    gm, levels, pool, err, records = model
    one = pool[:, 0].contiguous()
    if method == "acquire":
        return (lambda c, ws: gm.acquire(c, workspace=ws)), one, pool, gm.workspace_bytes(C)
    if method == "acquire_requests":
        return (lambda c, ws: gm.acquire_requests(c, workspace=ws)), pool, one, gm.workspace_bytes(C, S)
    if method == "acquire_topk":
        return (lambda c, ws: gm.acquire_topk(c, K, workspace=ws)), one, pool, gm.workspace_bytes_topk(C, K)
    if method == "logpdf":
        return (lambda c, ws: gm.logpdf(c, workspace=ws)), pool, one[0].contiguous(), gm.workspace_bytes_logpdf(S * C)
    return (lambda c, ws: gm.finish(c, records, err, levels, seed=5)), pool, one[0].contiguous(), None


@pytest.mark.parametrize("method", METHODS)
def test_refusals_leave_nothing_behind(model, device, method):
    import torch
    from hpbandster_amd import _native as N
    call, good, wrong_rank, wsb = _case(model, method)
    before = _arrays(call(good, None))
    swapped = good.transpose(-1, -2).contiguous().transpose(-1, -2)  # the pool's shape, the other memory order
    assert swapped.shape == good.shape and not swapped.is_contiguous()
    bad = {"float32": good.float(), "non-contiguous": swapped, "B + 1": torch.cat((good, good[:1])).contiguous(),
           "D - 1": good[..., :D - 1].contiguous(), "rank": wrong_rank}
    for what, cands in bad.items():
        with pytest.raises(N.HbxError):
            call(cands, None)
            pytest.fail("%s took a pool with %s" % (method, what))
    if wsb is not None:
        assert wsb > 0
        with pytest.raises(N.HbxError, match="workspace too small"):
            call(good, torch.empty(wsb - 1, dtype=torch.uint8, device=device))
        call(good, torch.empty(wsb, dtype=torch.uint8, device=device))  # exactly workspace_bytes* is enough
    after = _arrays(call(good, None))
    assert sorted(after) == sorted(before)
    for name in before:
        np.testing.assert_array_equal(after[name], before[name], err_msg="%s.%s" % (method, name))
