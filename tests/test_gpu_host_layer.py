"""The Python layer over the synchronous native calls: every way into KDEPair's one bound acquisition
(hbx_kde_acquire_bound) returns the same record, and DeviceKDE.sample's two ways to its one native call
(hbx_kde_sample) -- straight through on the model's device, or inside the device / stream context -- the same draws.
One small model throughout: 40 observations, 3 continuous + 2 categorical dims of 3 levels, min_points 6."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DC, DU, LEVELS, NOBS, MIN_POINTS = 3, 2, 3, 40, 6
FIELDS = ("index", "score", "pdf_l", "pdf_g", "shortlist", "near", "flags", "rel")


def _observations():
    from hpbandster_amd import synthetic as S
    return S.make_observations(NOBS, DC, DU, LEVELS, seed=61), S.make_losses(NOBS, seed=62)


def _fit(device):
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    X, losses = _observations()
    return kde.fit_pair(X, losses, S.var_type_string(DC, DU), MIN_POINTS, device=device)


@pytest.fixture(scope="module")
def pair(device):
    return _fit(device)


@pytest.mark.parametrize("Nc", [1, 64])
def test_sync_entry_forms_agree(device, pair, Nc):
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    C = S.make_candidates(Nc, DC, DU, LEVELS, seed=63)
    C_dev = torch.from_numpy(C).to(device)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    mapped = kde.mapped_candidates(Nc, DC + DU)
    mapped[...] = C
    ws = torch.empty(pair.workspace_bytes(Nc), dtype=torch.uint8, device=device)
    row = np.full(DC + DU, np.nan)
    fast = pair.acquire(C_dev)
    kept = pair._ws_cache[(threading.get_ident(), Nc)]
    recs = {"fast": fast,
            "numpy": pair.acquire(C),
            "stream": pair.acquire(C_dev, stream=side),
            "mapped": pair.acquire_mapped(mapped),
            "pick": pair.acquire_pick(C_dev, None, ws, row)}
    assert 0 <= fast.index < Nc
    for name, r in recs.items():
        for f in FIELDS:
            assert getattr(r, f) == getattr(fast, f), (name, f, r, fast)
    np.testing.assert_array_equal(row, C[fast.index])
    again = pair.acquire(C_dev)  # the fast path again, same thread: the kept workspace, not a new one
    assert again.index == fast.index
    assert pair._ws_cache[(threading.get_ident(), Nc)] is kept


def _bohb(device, num_samples):
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB
    space = CS.ConfigurationSpace(seed=4)
    for i in range(DC):
        space.add_hyperparameter(CS.UniformFloatHyperparameter("x%d" % i, lower=0, upper=1))
    for i in range(DU):
        space.add_hyperparameter(CS.CategoricalHyperparameter("y%d" % i, ["a", "b", "c"][:LEVELS]))
    cg = BOHB(space, min_points_in_model=MIN_POINTS, num_samples=num_samples, device=device, random_fraction=0.0,
              sampler="gpu", sampler_seed=42)

    class Job(object):
        pass

    X, losses = _observations()
    for k in range(NOBS):
        j = Job()
        j.id, j.exception, j.timestamps = (0, 0, k), None, {}
        j.kwargs = {"config": CS.Configuration(space, vector=X[k]).get_dictionary(), "budget": 1.0}
        j.result = {"loss": float(losses[k]), "info": None}
        cg.new_result(j)
    return cg


# (Nc, nobs) as the cases are named: nobs counts the model's observations.  The rule reads the good KDE's rows --
# 6 of the 40 here -- so both 64 and 256 draws reach 4 * 6 and use the Phi table; 16 draws stay below it.
@pytest.mark.parametrize("Nc", [64, 256, 16])
def test_sample_paths_agree(device, Nc):
    import torch
    good = _fit(device).good  # (a model of its own: whether a call built the table is read off it)
    assert good.nobs == 6
    lv = np.array([0] * DC + [LEVELS] * DU)
    bufs = (torch.empty((Nc, DC + DU), dtype=torch.float64, device=device),
            torch.empty(Nc, dtype=torch.int64, device=device), torch.empty(Nc, dtype=torch.uint8, device=device))
    with torch.cuda.device(device):
        out = good.sample(lv, 3.0, Nc, seed=7, counter_base=1000, out=bufs)  # no stream: straight through
    assert all(a is b for a, b in zip(out, bufs))
    assert (good._tab is not None) == (Nc >= 4 * good.nobs)
    torch.cuda.synchronize(device)
    direct = [t.cpu().numpy().tobytes() for t in bufs]
    side = torch.cuda.Stream(device=device)
    ctx = good.sample(lv, 3.0, Nc, seed=7, counter_base=1000, stream=side)  # inside the device and stream context
    side.synchronize()
    assert [t.cpu().numpy().tobytes() for t in ctx] == direct
    assert not np.frombuffer(direct[2], dtype=np.uint8).any()
    # two GPU-sampler generators, same seed and model, Nc draws per call, 5 get_config calls each: one on the
    # thread's default stream, one inside torch.cuda.stream(side) -- BOHB._pick then draws and acquires on a
    # stream that did not prepare the model and has to be ordered after it
    a, b = _bohb(device, Nc), _bohb(device, Nc)
    with torch.cuda.device(device):
        np.random.seed(3)
        plain = [a.get_config(1.0) for _ in range(5)]
        np.random.seed(3)
        with torch.cuda.stream(side):
            other = [b.get_config(1.0) for _ in range(5)]
    assert all(info["model_based_pick"] for _, info in plain)
    assert plain == other
    assert a._sample_counter == b._sample_counter == 5 * Nc
