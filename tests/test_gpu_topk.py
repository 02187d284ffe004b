"""Top-k acquisition (KDEPair.acquire_topk, hbx_kde_acquire_topk): the k best candidates of ONE pool must be
the first min(k, F) entries of the stable ascending order of the reference score max(1e-8, g)/max(l, 1e-8)
(bohb.py:129) over the F candidates whose score is not NaN -- index, score and both pdfs bit for bit.

The expected answer comes from the committed oracle alone: the split, bandwidths and level counts of
oracle.kde_oracle, the pdfs of c_oracle.kde_pdf(exact=True) (the pinned reference's float64 arithmetic),
kde_oracle.py_score, numpy's stable argsort.  No tolerances, no case skipped on a near-tie flag.  The pools are
built the way tests/test_gpu_fuzz.py builds its cases: quantised and clustered columns, observation rows and
perturbed ones as candidates, a duplicated row, a far block whose pdfs underflow so both factors clamp."""
import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

KS = (1, 2, 7, 64, 1024)
NCS = (1, 5, 257, 513, 700, 3000, 20000)  # 513/700: past the combine's 512-candidate block; > 1024: EXACT_SCAN_MAX


def _pool(seed, dc, du, nc, n=None):
    """Observations, losses, var_type, candidates, min_points_in_model (tests/test_gpu_fuzz.py::_case's
    recipe at fixed dims and pool size)."""
    rs = np.random.RandomState(7000 + seed)
    D = dc + du
    if n is None:
        n = int(rs.randint(200, 1000 if nc >= 20000 else 2000))
    levels = rs.randint(2, 7, size=du)
    X = np.empty((n, D))
    X[:, :dc] = rs.rand(n, dc)
    for d in range(dc):
        r = rs.rand()
        if r < 0.17:
            X[:, d] = np.round(X[:, d] * 8) / 8  # quantised: tied values
        elif r < 0.4:
            X[:, d] = 0.5 + 0.02 * rs.randn(n)  # clustered
    for u in range(du):
        X[:, dc + u] = rs.randint(0, levels[u], size=n)
    losses = rs.rand(n)
    if rs.rand() < 0.4:
        losses = np.round(losses * 20) / 20
    C = np.empty((nc, D))
    C[:, :dc] = rs.rand(nc, dc)
    for u in range(du):
        C[:, dc + u] = rs.randint(0, levels[u], size=nc)
    k = rs.rand(nc)
    src = X[rs.randint(0, n, size=nc)]
    cp = k < 0.2
    C[cp] = src[cp]  # observation rows as candidates
    pt = (k >= 0.2) & (k < 0.5)
    C[pt, :dc] = src[pt, :dc] + 0.01 * rs.randn(int(pt.sum()), dc)
    C[pt, dc:] = src[pt, dc:]
    far = (k >= 0.5) & (k < 0.6)
    C[far, :dc] = 4.0 + rs.rand(int(far.sum()), dc)  # pdfs underflow to 0
    if nc > 4:
        C[nc // 2] = C[nc // 4]  # a duplicate: an exact score tie
    return X, losses, "c" * dc + "u" * du, C, D + 1


def _oracle(X, losses, vt, C, mp):
    """(l, g, s, order): the oracle's pdfs and scores of every candidate and the stable ascending order of the
    non-NaN scores."""
    from oracle import c_oracle
    g_idx, b_idx = O.bohb_split(X, losses, mp)
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(X[g_idx], O.normal_reference_bw(X[g_idx]), vt, O.num_levels(X[g_idx], vt), C, exact=True)
        g = c_oracle.kde_pdf(X[b_idx], O.normal_reference_bw(X[b_idx]), vt, O.num_levels(X[b_idx], vt), C, exact=True)
    s = np.array([O.py_score(a, b) for a, b in zip(l, g)], dtype=np.float64)
    ok = np.nonzero(~np.isnan(s))[0]
    return l, g, s, ok[np.argsort(s[ok], kind="stable")]


def _check(top, ora, k, base=0, tag=None):
    l, g, s, order = ora
    want = order[:k]
    assert top.count == len(want) == len(top.index), (tag, top.count, len(want))
    np.testing.assert_array_equal(top.index, want + base, err_msg=str(tag))
    np.testing.assert_array_equal(top.score.view(np.int64), s[want].view(np.int64), err_msg=str(tag))
    np.testing.assert_array_equal(top.pdf_l, l[want], err_msg=str(tag))
    np.testing.assert_array_equal(top.pdf_g, g[want], err_msg=str(tag))
    assert top.shortlist >= top.count and top.rel.shape == (top.count,)


_cache = {}


def _fitted(device, key, build):
    """One pool per key for the whole module: (pair, C, oracle), computed once and left unchanged."""
    if key not in _cache:
        from hpbandster_amd import kde
        X, losses, vt, C, mp = build()
        _cache[key] = (kde.fit_pair(X, losses, vt, mp, device=device), C, _oracle(X, losses, vt, C, mp))
    return _cache[key]


# one seed per (shape, pool size), plus a second seed at the sizes on either side of EXACT_SCAN_MAX: 20 pools
SWEEP = [(dc, du, nc, 10 * i + (du > 0)) for i, nc in enumerate(NCS) for dc, du in ((8, 0), (13, 3))] + \
        [(dc, du, nc, 100 + j) for j, (dc, du, nc) in enumerate([(8, 0, 700), (13, 3, 700), (8, 0, 3000), (13, 3, 3000),
                                                                (8, 0, 513), (13, 3, 257)])]


@pytest.mark.parametrize("dc,du,nc,seed", SWEEP)
def test_topk_matches_oracle(device, dc, du, nc, seed):
    """Every k of the sweep (k > Nc included) on one pool; k = 1 is also acquire()'s pick field for field."""
    pair, C, ora = _fitted(device, ("sweep", dc, du, nc, seed), lambda: _pool(seed, dc, du, nc))
    for k in KS:
        _check(pair.acquire_topk(C, k), ora, k, tag=(dc, du, nc, seed, k))
    top, one = pair.acquire_topk(C, 1), pair.acquire(C)
    assert top.count == 1
    assert (int(top.index[0]), float(top.score[0]), float(top.pdf_l[0]), float(top.pdf_g[0])) == \
        (one.index, one.score, one.pdf_l, one.pdf_g)
    assert float(top.rel[0]) == np.float32(one.rel)


def test_ties_at_the_boundary(device):
    """The pool's best row 40 times at scattered indices: every k from 1 to 45 cuts through (or just past) the run
    of equal scores, whose indices must come out smallest first."""
    def build():
        X, losses, vt, C, mp = _pool(31, 8, 0, 700)
        best = int(_oracle(X, losses, vt, C, mp)[3][0])
        at = np.random.RandomState(5).choice(np.setdiff1d(np.arange(700), [best]), 39, replace=False)
        C[at] = C[best]
        return X, losses, vt, C, mp
    pair, C, ora = _fitted(device, "ties", build)
    l, g, s, order = ora
    run = order[:40]
    assert np.all(s[run] == s[run[0]]) and np.all(np.diff(run) > 0) and s[order[40]] > s[run[0]]
    assert run[-1] - run[0] > 300  # scattered over the pool
    for k in range(1, 46):
        _check(pair.acquire_topk(C, k), ora, k, tag=k)


def test_score_exactly_one(device):
    """2900 of 3000 candidates where both pdfs underflow: their score is exactly 1e-8/1e-8 = 1, a tie the argmin
    represents by its first member only; the top-k cut falls inside it."""
    def build():
        X, losses, vt, C, mp = _pool(32, 8, 0, 3000)
        rs = np.random.RandomState(6)
        C[100:] = 4.0 + rs.rand(2900, 8)
        return X, losses, vt, C, mp
    pair, C, ora = _fitted(device, "ones", build)
    l, g, s, order = ora
    assert np.all(s[100:] == 1.0)
    below = int(np.sum(s[:100] < 1.0))
    assert below < 64  # both cuts fall inside the block of ones
    for k in (64, 300):
        top = pair.acquire_topk(C, k)
        _check(top, ora, k, tag=k)
        assert np.all(top.score[below:] == 1.0)


def test_fewer_than_k_rankable(device):
    """A constant continuous column (bandwidth 0: every score NaN) returns nothing; a categorical dim with a
    single observed level in ONE KDE follows the reference's asymmetry: NaN l -> NaN score (never returned),
    NaN g -> max(1e-8, NaN) = 1e-8 (ranked)."""
    def const():
        X, losses, vt, C, mp = _pool(33, 8, 0, 700)
        X[:, 2] = 0.25
        return X, losses, vt, C, mp
    pair, C, ora = _fitted(device, "const", const)
    assert len(ora[3]) == 0
    for k in (1, 64):
        top = pair.acquire_topk(C, k)
        assert top.count == 0 and top.index.size == 0 and top.score.size == 0
    for which in (0, 1):
        def single():
            X, losses, vt, C, mp = _pool(34 + which, 13, 3, 700)
            rows = O.bohb_split(X, losses, mp)[which]
            X[rows, 14] = 1.0  # this KDE sees one level of dim 14; the other several
            return X, losses, vt, C, mp
        pair, C, ora = _fitted(device, ("single", which), single)
        F = len(ora[3])
        assert (0 < F < 700) if which == 0 else F == 700
        for k in (7, 1024):
            top = pair.acquire_topk(C, k)
            assert top.count == min(k, F)
            _check(top, ora, k, tag=(which, k))


@pytest.mark.parametrize("family", ["exact_only", "signed", "f32"])
def test_other_kernel_families(device, family):
    """KDEs outside every fp32 bucket (65 continuous dims: every candidate re-scored), with a negative
    Aitchison-Aitken match factor (a categorical bandwidth > 1: signed sums), and on the f32 scoring kernel
    (3 continuous dims)."""
    from hpbandster_amd import synthetic as S

    def build():
        if family == "exact_only":
            return _pool(40, 65, 0, 300, n=200)
        if family == "f32":
            return _pool(41, 3, 0, 700)
        X = S.make_observations(40, 2, 3, 10)
        C = S.make_candidates(400, 2, 3, 10)
        C[:200, 2:] = X[np.random.RandomState(9).randint(0, 40, 200)][:, 2:]
        return X, S.make_losses(40), S.var_type_string(2, 3), C, 6
    pair, C, ora = _fitted(device, family, build)
    if family == "exact_only":
        assert (pair.good.variant >> 5) & 1
    if family == "signed":
        assert max(pair.good.bw[2:].max(), pair.bad.bw[2:].max()) > 1.0
    for k in (1, 10, 64):
        top = pair.acquire_topk(C, k)
        _check(top, ora, k, tag=(family, k))
        if family == "exact_only":
            assert top.shortlist == len(C)


@pytest.mark.parametrize("k", [1, 64])
def test_sharded_merge_equals_whole_pool(device, k):
    """8 contiguous shards with index_base, merged on the host: the whole pool's top-k exactly."""
    import torch
    from hpbandster_amd.distributed import merge_topk, shard_range
    dc, du, nc, seed = SWEEP[12]
    assert (dc, du, nc) == (8, 0, 20000)
    pair, C, ora = _fitted(device, ("sweep", dc, du, nc, seed), lambda: _pool(seed, dc, du, nc))
    Cd = torch.from_numpy(C).to(device)
    parts = []
    for r in range(8):
        lo, hi = shard_range(nc, r, 8)
        parts.append(pair.acquire_topk(Cd[lo:hi], k, index_base=lo))
    whole, merged = pair.acquire_topk(Cd, k), merge_topk(parts, k)
    _check(merged, ora, k)
    for f in ("index", "score", "pdf_l", "pdf_g", "rel"):
        np.testing.assert_array_equal(getattr(merged, f), getattr(whole, f))
    assert merged.count == whole.count == k


def test_generator_topk(device):
    """BOHB.get_config_topk: entry 0 is get_config's model-based pick from the same RNG state, and the global
    RNG ends where that get_config leaves it."""
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB
    space = CS.ConfigurationSpace(seed=3)
    for i in range(3):
        space.add_hyperparameter(CS.UniformFloatHyperparameter("x%d" % i, lower=-2, upper=3))
    space.add_hyperparameter(CS.CategoricalHyperparameter("c", ["a", "b", "c", "d"]))
    # random_fraction 0: get_config's draw always goes model-based
    cg = BOHB(space, device=device, random_fraction=0.0, num_samples=32, sampler="host")
    assert cg.get_config_topk(1.0, 8) == []  # no model yet

    class Job(object):
        pass

    rs = np.random.RandomState(3)
    for k in range(40):
        j = Job()
        j.id, j.exception, j.timestamps = (0, 0, k), None, {}
        j.kwargs = {"config": space.sample_configuration().get_dictionary(), "budget": 1.0}
        j.result = {"loss": float(rs.rand()), "info": None}
        cg.new_result(j)
    assert len(cg.kde_models) == 1
    np.random.seed(7)
    one, info = cg.get_config(1.0)
    assert info["model_based_pick"]
    after = np.random.get_state()
    np.random.seed(7)
    top = cg.get_config_topk(1.0, 8)
    got = np.random.get_state()
    np.testing.assert_array_equal(got[1], after[1])
    assert got[2:] == after[2:]
    assert 1 <= len(top) <= 8
    assert top[0][0] == one
    scores = [i["score"] for _, i in top]
    assert all(i["model_based_pick"] for _, i in top) and scores == sorted(scores)
    with pytest.raises(ValueError):
        cg.get_config_topk(1.0, 0)


def test_arguments_and_side_stream(device):
    import torch
    from hpbandster_amd import _native as N
    dc, du, nc, seed = SWEEP[8]
    assert nc == 700
    pair, C, ora = _fitted(device, ("sweep", dc, du, nc, seed), lambda: _pool(seed, dc, du, nc))
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            pair.acquire_topk(C, bad)
    with pytest.raises(ValueError):
        pair.acquire_topk(C, 4, ties="process")
    with pytest.raises(N.HbxError):
        pair.acquire_topk(np.zeros((4, dc + du + 1)), 2)
    empty = pair.acquire_topk(np.empty((0, dc + du)), 5)
    assert empty.count == 0 and empty.shortlist == 0 and empty.index.size == 0
    side = torch.cuda.Stream(device=device)
    Cd = torch.from_numpy(C).to(device)
    torch.cuda.synchronize(device)
    _check(pair.acquire_topk(Cd, 7, stream=side), ora, 7)
    ws = torch.empty(pair.topk_workspace_bytes(nc, 64), dtype=torch.uint8, device=device)
    _check(pair.acquire_topk(Cd, 64, workspace=ws), ora, 64)  # a caller's workspace, reused
    _check(pair.acquire_topk(Cd, 2, workspace=ws), ora, 2)
