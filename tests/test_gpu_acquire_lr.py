"""Single-pool acquisition by log ratio (hbx_kde_acquire_lr, hbx_kde_acquire_bound_lr; KDEPair.acquire(score="log_ratio"),
BOHB(score="log_ratio")) on the GPU against a reference built here from the oracle, as tests/test_gpu_groups_lr.py
builds it: c_oracle.kde_pdf(exact=True) for both pdfs (the reference's arithmetic); per KDE L = log(p) for a positive
normal pdf, NaN for a negative or NaN one, the oracle's log-space value where p underflowed in a KDE without a negative
match factor and log(p) as it is otherwise; s = L_g - L_l in fp64; the winner by (s, index), NaN never.

Candidate counts: 5 one partial tile; 130; 1030 past EXACT_SCAN_MAX (a shortlist launch of its own); 70 000 past the
65 536 below which scoring launches split (5 .. 1030 run split at the larger models, 70 000 unsplit).  Every case is
decided: the reference's gap between the best and the runner-up exceeds both tolerances (asserted first)."""
import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

NEAR_TIE, OVERFLOW, LOG_RATIO = 2, 1, 128
COUNTS = [5, 130, 1030, 70000]
#        dc, du, levels, rows
KINDS = {"d1": (1, 0, 0, 40), "c8": (8, 0, 0, 60), "c3u2": (3, 2, 3, 120), "signed": (24, 8, 4, 240),
         "under": (3, 2, 3, 120), "exact": (3, 2, 3, 120)}
TINY = np.finfo(np.float64).tiny
FAR = 48  # under: the pool's first candidates lie far from the cluster, each at its own distance
_MODELS, _REFS = {}, {}


def _observations(kind):
    """under: the continuous columns are clustered within 1e-3, so the bandwidths are tiny; exact: the last categorical
    column holds a single level (with a minimum bandwidth the pair is exact-only)"""
    dc, du, nl, n = KINDS[kind]
    rs = np.random.RandomState(len(kind) + dc)
    cont = rs.rand(n, dc) if kind != "under" else 0.5 + 1e-3 * rs.randn(n, dc)
    X = np.concatenate((cont, rs.randint(0, max(nl, 1), size=(n, du)).astype(np.float64)), axis=1)
    if kind == "exact":
        X[:, -1] = 1.0
    return X, rs.rand(n), "c" * dc + "u" * du


def _model(device, kind):
    from hpbandster_amd import kde
    if kind not in _MODELS:
        X, losses, vt = _observations(kind)
        pair = kde.fit_pair(X, losses, vt, len(vt) + 1, device=device, min_bandwidth=1e-3 if kind == "exact" else None)
        dc = KINDS[kind][0]
        assert kind != "signed" or np.any(pair.good.bw[dc:] > 1.0)  # few good rows: the good KDE is signed
        _MODELS[kind] = (pair, vt, [(k.data, k.bw, k.nlev) for k in (pair.good, pair.bad)])
    return _MODELS[kind]


def _pool(kind, C, seed=0):
    dc, du, nl, _ = KINDS[kind]
    rs = np.random.RandomState(1000 * len(kind) + C + seed)
    pool = np.concatenate((rs.rand(C, dc), rs.randint(0, max(nl, 1), size=(C, du))), axis=1).astype(np.float64)
    if kind == "under":  # near the cluster, except the first FAR candidates
        pool[:, :dc] = 0.5 + 2e-3 * rs.randn(C, dc)
        dist = rs.uniform(0.15, 0.4, size=(min(C, FAR), 1))
        dist[0] = 0.1
        pool[:FAR, :dc] = 0.5 + dist * np.sign(rs.randn(min(C, FAR), dc))
    pool[1, 0] = np.nan  # a NaN coordinate is never picked
    return pool


def _reference(kdes, vt, x):
    """per candidate of x [C, D]: s_ref, the tolerance of s, both oracle pdfs, whether an L took the log-space route"""
    from oracle import c_oracle
    cont = np.array([c == "c" for c in vt])
    out = []
    for data, bw, nlev in kdes:
        with np.errstate(all="ignore"):
            p = c_oracle.kde_pdf(data, bw, vt, nlev, x, exact=True)
            L = np.where((p != p) | (p < 0), np.nan, np.log(p))
            under = (p >= 0) & (p < TINY) & ~np.any(bw[~cont] > 1.0)
            ls = np.zeros(len(x))
            if under.any():
                xu = x[under]
                L[under] = O.log_pdf_many(data, bw, vt, xu, nlev)
                # the kernel's bound of the log-space value, (D + 2) 2^-53 max|t| + (n + 256) 2^-52, with the pairs' t
                # from the fitted bandwidths: -d^2 / (2 h^2) per continuous dim, ln of the match factor per categorical
                hu, cu = bw[~cont], np.asarray(nlev)[~cont]
                lm, ln_ = np.log(np.abs(1 - hu)), np.log(hu / (cu - 1))
                t = [-np.sum((data[:, cont] - xi[cont]) ** 2 / (2 * bw[cont] ** 2), axis=1) +
                     np.sum(np.where(data[:, ~cont] == xi[~cont], lm, ln_), axis=1) for xi in xu]
                tmax = np.array([np.max(np.abs(ti[np.isfinite(ti)]), initial=0.0) for ti in t])
                ls[under] = 4 * ((len(vt) + 2) * 2.0 ** -53 * tmax + (len(data) + 256) * 2.0 ** -52)
        out.append((p, L, ls, under))
    (pl, Ll, el, ul), (pg, Lg, eg, ug) = out
    # the score's tolerance: 8 2^-53 max(1, |L_l|, |L_g|) on the exact route (two logs of at most 1 ulp and a
    # subtraction), and four times the log-space bound of each L that took that route
    mag = np.maximum(np.nan_to_num(np.abs(Ll), nan=0.0, posinf=1.0), np.nan_to_num(np.abs(Lg), nan=0.0, posinf=1.0))
    with np.errstate(all="ignore"):
        return Lg - Ll, 8 * 2.0 ** -53 * np.maximum(1.0, mag) + el + eg, pl, pg, ul | ug


def _decided_winner(s, tol):
    """the first index of the smallest s, NaN never; asserts that the runner-up lies beyond both tolerances"""
    ok = np.flatnonzero(~np.isnan(s))
    assert len(ok)
    win = int(ok[np.argmin(s[ok])])
    rest = ok[ok != win]
    if len(rest):
        run = int(rest[np.argmin(s[rest])])
        assert s[run] - s[win] > tol[run] + tol[win], (win, run, s[win], s[run])
    return win


def _case(device, kind, C):
    pair, vt, kdes = _model(device, kind)
    if (kind, C) not in _REFS:
        pool = _pool(kind, C)
        _REFS[kind, C] = (pool,) + _reference(kdes, vt, pool)
    return (pair,) + _REFS[kind, C]


def _check(r, win, s, tol, pl, pg, tag):
    print(tag, "index", r.index, "ref", win, "score", r.score, "shortlist", r.shortlist, "near", r.near, "flags", r.flags)
    assert r.index == win and r.index != 1, tag
    assert np.float64(r.pdf_l).tobytes() == pl[win].tobytes() and np.float64(r.pdf_g).tobytes() == pg[win].tobytes(), tag
    assert r.score == s[win] or abs(r.score - s[win]) <= tol[win], (tag, r.score, s[win], tol[win])
    assert r.flags & LOG_RATIO and r.shortlist >= 1, tag


@pytest.mark.parametrize("C", COUNTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pick_equals_the_reference(device, kind, C):
    pair, pool, s, tol, pl, pg, under = _case(device, kind, C)
    win = _decided_winner(s, tol)
    r = pair.acquire(pool, score="log_ratio")
    _check(r, win, s, tol, pl, pg, (kind, C))
    assert bool(r.flags & OVERFLOW) == (kind == "exact"), (kind, C)  # exact-only: the whole pool re-scored
    if kind == "under":  # the far candidates' exact g is 0: the log-space argmin, not the lowest index
        assert np.sum(pg[:FAR] == 0.0) >= 3 and under[win] and win != 0, (kind, C)


def test_no_score_and_empty_pool(device):
    pair, pool, *_ = _case(device, "c3u2", 130)
    for cands in (np.full_like(pool, np.nan), pool[:0]):
        r = pair.acquire(cands, score="log_ratio")
        assert r.index == -1 and np.isnan(r.score) and r.flags & LOG_RATIO, r
        assert len(cands) or (r.shortlist == 0 and r.near == 0)


def test_the_floored_score_ties_where_the_log_ratio_decides(device):
    """24c + 8u, a pool of uniform draws over the box [-1, 2)^24 (about what the generator's own sampler covers at three
    bandwidths; over [0, 1) alone a few of 256 candidates reach 1e-6): every candidate's l and g lie under the floor,
    the floored score is exactly 1 and its argmin the first candidate; s = ln g - ln l still orders the pool"""
    pair, vt, kdes = _model(device, "signed")
    rs = np.random.RandomState(0)
    pool = np.concatenate((3 * rs.rand(256, 24) - 1, rs.randint(0, 4, size=(256, 8))), axis=1).astype(np.float64)
    pool[1, 0] = np.nan
    s, tol, pl, pg, _ = _reference(kdes, vt, pool)
    win = _decided_winner(s, tol)
    assert win != 0 and np.nanmax(pl) < 1e-8 and np.nanmax(pg) < 1e-8
    floored = pair.acquire(pool)
    assert floored.index == 0 and floored.score == 1.0 and not floored.flags & LOG_RATIO
    _check(pair.acquire(pool, score="log_ratio"), win, s, tol, pl, pg, "signed/rand")


@pytest.mark.parametrize("kind,C", [("c3u2", 130), ("under", 1030)])
def test_bound_call_equals_the_unbound_call(device, kind, C):
    import torch
    from hpbandster_amd import kde
    pair, pool, s, tol, pl, pg, _ = _case(device, kind, C)
    cands = torch.from_numpy(pool).to(device)
    unbound = kde.AcqResult.from_bytes(pair.acquire(cands, sync=False, score="log_ratio").cpu().numpy().tobytes())
    ws = torch.empty(pair.workspace_bytes(C, "log_ratio"), dtype=torch.uint8, device=device)
    row = np.full(pool.shape[1], -1.0)
    picked = pair.acquire_pick(cands, torch.zeros(C, dtype=torch.uint8, device=device), ws, row, score="log_ratio")
    _check(unbound, _decided_winner(s, tol), s, tol, pl, pg, (kind, C, "unbound"))
    fields = kde.AcqResult.__slots__
    assert [getattr(picked, f) for f in fields] == [getattr(unbound, f) for f in fields]
    assert row.tobytes() == pool[unbound.index].tobytes()


@pytest.mark.parametrize("sampler", ["host", "gpu"])
def test_generator_picks_by_log_ratio(device, sampler):
    """BOHB(score="log_ratio").get_config on a seeded 24c + 8u run against a host restatement: the same draws, then the
    reference pick"""
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB
    space = CS.ConfigurationSpace(seed=3)
    for i in range(24):
        space.add_hyperparameter(CS.UniformFloatHyperparameter("x%02d" % i, lower=0, upper=1))
    for i in range(8):
        space.add_hyperparameter(CS.CategoricalHyperparameter("z%d" % i, ["a", "b", "c", "d"]))
    cg = BOHB(space, device=device, random_fraction=0.0, sampler=sampler, sampler_seed=5, score="log_ratio")

    class Job(object):
        pass

    rs = np.random.RandomState(3)
    for k in range(120):
        j = Job()
        j.id, j.exception, j.timestamps = (0, 0, k), None, {}
        j.kwargs = {"config": space.sample_configuration().get_dictionary(), "budget": 1.0}
        j.result = {"loss": float(rs.rand()), "info": None}
        cg.new_result(j)
    pair = cg.kde_models[1.0]
    np.random.seed(7)
    got, info = cg.get_config(1.0)
    assert info["model_based_pick"] and cg._sample_counter == (cg.num_samples if sampler == "gpu" else 0)
    np.random.seed(7)
    np.random.rand()  # get_config's random_fraction draw
    if sampler == "gpu":
        cands = pair.good.sample(cg.vartypes, cg.bw_factor, cg.num_samples, cg.sampler_seed, 0)[0].cpu().numpy()
    else:
        cands = cg.sample_candidates(pair.good, cg.num_samples)
    s, tol, _, _, _ = _reference([(k.data, k.bw, k.nlev) for k in (pair.good, pair.bad)], cg.kde_vartypes, cands)
    win = _decided_winner(s, tol)
    print(sampler, "winner", win, "s", s[win])
    assert got == cg._to_dict(cands[win])
