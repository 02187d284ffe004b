"""The staged top-k acquisition (hbx_topk.hip "Staged scoring", hbx_staged.hip's launches): the good KDE scored
for every candidate, the bad KDE only for the candidates that can still rank among the k best -- the seeds around
the (k+1)-th largest l and the candidates whose l-only bound 1e-8 / max(l, 1e-8) does not exceed the seeds'
(k+1)-th smallest upper score bound.

Every case runs the same pair, candidates and workspace with HBX_STAGED=2 (staged wherever supported) and
HBX_STAGED=0 (never) and compares `count`, `flags` and the bytes of `index`, `score`, `pdf_l`, `pdf_g`, `rel`;
`shortlist` describes the screen and may differ.  The ranking is checked against the C oracle with
tests/test_gpu_topk.py's _check, and KDEPair.acquire_stats proves which branch a case reached.  Pairs are fitted
as in tests/test_gpu_staged.py (categorical bandwidths capped at 0.8: unsigned KDEs, the coarse instance).
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_row_stage import _coarse, _pair
from tests.test_gpu_staged import CAP, _fit
from tests.test_gpu_topk import _check

pytestmark = pytest.mark.gpu

FIELDS = ("index", "score", "pdf_l", "pdf_g", "rel")
OVERFLOW, NEAR_TIE = 1, 2


def _oracle(pair, vt, C):
    """(l, g, s, order) as tests/test_gpu_topk.py's _oracle gives them, from a fitted pair's rows and bandwidths."""
    from oracle import c_oracle
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    s = np.array([O.py_score(a, b) for a, b in zip(l, g)], dtype=np.float64)
    ok = np.nonzero(~np.isnan(s))[0]
    return l, g, s, ok[np.argsort(s[ok], kind="stable")]


def _equal(on, off, shortlist=False):
    assert (on.count, on.flags) == (off.count, off.flags), (on, off)
    for f in FIELDS:
        assert getattr(on, f).tobytes() == getattr(off, f).tobytes(), (f, on, off)
    if shortlist:
        assert on.shortlist == off.shortlist, (on, off)


def _both(pair, C, k, monkeypatch, device, expect_staged=True, base=0):
    """(staged block, its stats, unstaged block) of one pool on one workspace; the stats of each call its own."""
    import torch
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    nc = len(C)
    ws = torch.empty(pair.topk_workspace_bytes(nc, k), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "2")
    on = pair.acquire_topk(Cd, k, index_base=base, workspace=ws)
    st = pair.acquire_stats(ws, nc)
    assert st["staged"] == expect_staged, st
    monkeypatch.setenv("HBX_STAGED", "0")
    off = pair.acquire_topk(Cd, k, index_base=base, workspace=ws)
    st0 = pair.acquire_stats(ws, nc)
    assert not st0["staged"] and st0["evaluated"] == nc, st0
    _equal(on, off, shortlist=not expect_staged)
    return on, st, off


N_NEAR, N_FAR = 2048, 2049


def _prune_pool(pair, rs):
    """4097 candidates, shuffled: 2048 good observation rows moved by 0.01 sigma per continuous dim (l large, g
    small) and 2049 rows far from the data (4 + U[0, 1) per continuous dim: both pdfs underflow)."""
    good = pair.good.data
    near = good[rs.randint(0, len(good), size=N_NEAR)].copy()
    near[:, :24] += 0.01 * rs.randn(N_NEAR, 24)
    far = good[rs.randint(0, len(good), size=N_FAR)].copy()
    far[:, :24] = 4.0 + rs.rand(N_FAR, 24)
    perm = rs.permutation(N_NEAR + N_FAR)
    C = np.vstack([near, far])[perm]
    is_far = (np.arange(N_NEAR + N_FAR) >= N_NEAR)[perm]
    return np.ascontiguousarray(C), is_far


@pytest.fixture(scope="module")
def prune(device):
    """24c + 8u (tests/test_gpu_row_stage.py's `wide` pair) with _prune_pool and the oracle's values."""
    pair, vt = _pair(24, 8, 4, 311, device)
    assert _coarse(pair)
    C, is_far = _prune_pool(pair, np.random.RandomState(411))
    ora = _oracle(pair, vt, C)
    l, g, s, order = ora
    assert int(np.sum(s < 0.5)) >= 1025  # k + 1 certain scores below 1 for every k
    assert np.all(l[is_far] < 1e-9) and int(is_far.sum()) == N_FAR > len(C) // 2
    return pair, vt, C, is_far, ora


@pytest.mark.parametrize("k", [1, 2, 64, 1024])
def test_prunes(device, monkeypatch, prune, k):
    """4097 candidates (the seeds' gather crosses a tile boundary), index base 5 * 2^32.  At least k + 1 candidates
    score below 0.5, so k + 1 seeds have an upper bound below ln 1 = 0, while every far candidate's l lies below
    the clamp by hundreds of ln units and its l-only bound is exactly 0: each far candidate must be pruned."""
    pair, vt, C, is_far, ora = prune
    base = 5 * 2 ** 32
    on, st, off = _both(pair, C, k, monkeypatch, device, base=base)
    print("staged top-k stats", k, st, "shortlist", on.shortlist, off.shortlist)
    _check(on, ora, k, base=base, tag=k)
    assert st["evaluated"] <= len(C) - N_FAR, st
    assert st["seeds"] >= k + 1, st


@pytest.mark.parametrize("k", [1, 64])
def test_nothing_pruned(device, monkeypatch, k):
    """8 continuous dims, 1537 candidates near the data: every pdf far above 1e-8, every l-only bound far below
    any real score -- every candidate is evaluated."""
    from hpbandster_amd import synthetic as S
    pair, vt = _pair(8, 0, 1, 331, device)
    assert _coarse(pair)
    C = S.make_candidates(1537, 8, 0, 1, seed=333)
    on, st, off = _both(pair, C, k, monkeypatch, device)
    ora = _oracle(pair, vt, C)
    assert ora[0].min() > 1e-6  # the premise
    _check(on, ora, k)
    assert st["evaluated"] == len(C), st


def test_band_larger_than_the_list(device, monkeypatch):
    """16 continuous dims, 8300 candidates within 0.05 of good observations, k = 1024: the seed list is full and
    more than 4096 survivors run unsplit."""
    pair, vt = _pair(16, 0, 1, 341, device)
    assert _coarse(pair)
    rs = np.random.RandomState(343)
    C = pair.good.data[rs.randint(0, len(pair.good.data), size=8300)] + 0.05 * rs.randn(8300, 16)
    on, st, off = _both(pair, C, 1024, monkeypatch, device)
    assert st["seeds"] == CAP and st["survivors"] > CAP, st
    _check(on, _oracle(pair, vt, C), 1024)


def test_fewer_than_k_plus_one_rankable(device, monkeypatch, prune):
    """k >= Nc, k = Nc - 1, and rows holding NaN in a continuous and in a categorical column: no (k+1)-th l, so no
    threshold -- nothing is pruned and count = F, the number of candidates with a score."""
    pair, vt, C, is_far, ora = prune
    for nc, k in ((700, 1024), (700, 700), (65, 64)):
        sub = C[:nc]
        o = _oracle(pair, vt, sub)
        F = len(o[3])
        on, st, off = _both(pair, sub, k, monkeypatch, device)
        _check(on, o, k, tag=(nc, k))
        assert on.count == min(k, F) and st["evaluated"] == nc, (nc, k, st)
    sub = C[:700].copy()
    sub[5, 3] = np.nan
    sub[130, 0] = np.nan
    sub[40, 27] = np.nan
    o = _oracle(pair, vt, sub)
    F = len(o[3])
    assert F < 700
    on, st, off = _both(pair, sub, 1024, monkeypatch, device)
    _check(on, o, 1024, tag="nan")
    assert on.count == F and st["evaluated"] >= F, st
    assert not set(on.index.tolist()) & {5, 130}


def test_duplicates_straddle_rank_k(device, monkeypatch, prune):
    """The row at rank k - 1 copied over four far rows at scattered indices: the copies take ranks k - 1 .. k + 3,
    and the two returned ones are the lowest indices."""
    pair, vt, C, is_far, ora = prune
    k = 8
    C = C.copy()
    src = int(ora[3][k - 2])
    at = np.nonzero(is_far)[0][[3, 500, 1200, 2000]]
    C[at] = C[src]
    o = _oracle(pair, vt, C)
    copies = np.sort(np.concatenate([[src], at]))
    assert set(o[3][k - 2:k + 3].tolist()) == set(copies.tolist())
    on, st, off = _both(pair, C, k, monkeypatch, device)
    _check(on, o, k)
    assert on.index[k - 2:].tolist() == copies[:2].tolist()


@pytest.mark.parametrize("k", [1, 64])
def test_every_score_exactly_one(device, monkeypatch, prune, k):
    """Every candidate far from the data: every score is exactly 1e-8 / 1e-8.  U_(k+1)_seed = 0 and every l-only
    bound is 0 too: nothing may be pruned, and the first k indices come back."""
    pair, vt, C, is_far, ora = prune
    sub = np.ascontiguousarray(C[is_far][:700])
    on, st, off = _both(pair, sub, k, monkeypatch, device)
    assert on.index.tolist() == list(range(k)) and np.all(on.score == 1.0)
    assert st["evaluated"] == len(sub), st
    _check(on, _oracle(pair, vt, sub), k)


def test_fewer_than_k_below_one(device, monkeypatch, prune):
    """m = 5 candidates scoring below 1 among 695 exact ones, k = 16: the 5, then the first 11 exact ones by
    index."""
    pair, vt, C, is_far, ora = prune
    l, g, s, order = ora
    m, k = 5, 16
    sub = np.ascontiguousarray(C[is_far][:700])
    put = [17, 90, 333, 512, 699]
    sub[put] = C[order[:m]]
    o = _oracle(pair, vt, sub)
    assert int(np.sum(o[2] < 1.0)) == m and int(np.sum(o[2] == 1.0)) == 700 - m
    on, st, off = _both(pair, sub, k, monkeypatch, device)
    _check(on, o, k)
    assert sorted(on.index[:m].tolist()) == put
    assert on.index[m:].tolist() == [i for i in range(700) if i not in put][:k - m]


@pytest.mark.parametrize("name", ["neartie_c", "neartie_m"])
def test_near_tie_flag(device, monkeypatch, name):
    """The near-tie fixtures at k = 1, 2, 4: HBX_ACQ_NEAR_TIE (the last returned entry against the best excluded
    one included) is the same in both modes."""
    import torch
    from hpbandster_amd import kde
    from tests import golden_cases as G
    c = G.load_kde_case(name)
    pair = kde.fit_pair_from_rows(c["X"], c["good_idx"], c["bad_idx"], c["var_type"], c["bw_good"], c["bw_bad"],
                                  c["nlev_good"], c["nlev_bad"], device=device)
    C = np.ascontiguousarray(c["cands"])
    Cd = torch.from_numpy(C).to(device)
    for k in (1, 2, 4):
        ws = torch.empty(pair.topk_workspace_bytes(len(C), k), dtype=torch.uint8, device=device)
        monkeypatch.setenv("HBX_STAGED", "2")
        on = pair.acquire_topk(Cd, k, workspace=ws)
        monkeypatch.setenv("HBX_STAGED", "0")
        off = pair.acquire_topk(Cd, k, workspace=ws)
        _equal(on, off)
        assert (on.flags & NEAR_TIE) == (off.flags & NEAR_TIE)
    assert on.index[0] == c["chosen"]


def test_overflow_from_l(device, monkeypatch):
    """tests/test_gpu_staged_tail.py's test_overflow_from_l: ln l is about 707 at the good rows, past the overflow
    flag's 700, and underflows 1e-18 away.  Both modes set HBX_ACQ_OVERFLOW and re-score every candidate."""
    rs = np.random.RandomState(331)
    n, D, nc = 400, 16, 300
    X = 1e-19 * rs.rand(n, D)
    losses = rs.rand(n)
    pair = _fit(X, losses, "c" * D, device, bw_good=lambda bw: np.full(D, 2e-20), bw_bad=lambda bw: np.full(D, 1e-10))
    g_idx, _ = O.bohb_split(X, losses, D + 1)
    C = np.vstack([X[g_idx][rs.randint(0, len(g_idx), size=nc // 2)], 1e-18 + 1e-19 * rs.rand(nc - nc // 2, D)])
    on, st, off = _both(pair, C[rs.permutation(nc)], 8, monkeypatch, device)
    assert on.flags & OVERFLOW and off.flags & OVERFLOW
    assert on.shortlist == off.shortlist == nc


def test_overflow_guard_of_the_bad_kde(device, monkeypatch):
    """The same 16 dims with the bad KDE's bandwidths at 2e-18: its largest attainable ln pdf, 16 (40.75 - 0.92) =
    637, lies within 100 of the flag's 700, so U_(k+1)_seed stays +inf and every candidate is evaluated, the ones
    whose l underflows (1e-8 away, under good bandwidths of 1e-10) included."""
    rs = np.random.RandomState(337)
    n, D, nc = 400, 16, 300
    X = 1e-19 * rs.rand(n, D)
    losses = rs.rand(n)
    pair = _fit(X, losses, "c" * D, device, bw_good=lambda bw: np.full(D, 1e-10), bw_bad=lambda bw: np.full(D, 2e-18))
    g_idx, _ = O.bohb_split(X, losses, D + 1)
    C = np.vstack([X[g_idx][rs.randint(0, len(g_idx), size=nc // 2)], 1e-8 + 1e-19 * rs.rand(nc - nc // 2, D)])
    on, st, off = _both(pair, C[rs.permutation(nc)], 8, monkeypatch, device)
    assert st["evaluated"] == nc, st


def test_unsupported_pairs(device, monkeypatch, prune):
    """HBX_STAGED=2 on calls the staged path does not serve -- a signed good KDE, an exact-only pair, HBX_COARSE=0
    -- runs the unstaged path: the stats say so and the whole block is equal, `shortlist` included."""
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    from tests.test_gpu_topk import _pool
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=271)
    signed = _fit(X, S.make_losses(400, seed=272), vt, device, cat_bw=None,
                  bw_good=lambda bw: np.concatenate([bw[:24], np.full(8, 1.2)]))
    assert signed.good.has_neg
    _both(signed, S.make_candidates(900, 24, 8, 4, seed=273), 7, monkeypatch, device, expect_staged=False)
    Xe, le, vte, Ce, mpe = _pool(40, 65, 0, 300, n=200)
    exact = kde.fit_pair(Xe, le, vte, mpe, device=device)
    assert (exact.good.variant >> 5) & 1
    _both(exact, Ce, 7, monkeypatch, device, expect_staged=False)
    pair, vt, C, is_far, ora = prune
    monkeypatch.setenv("HBX_COARSE", "0")  # (read when a KDE is prepared: no coarse table, no coarse instance)
    plain, _ = _pair(24, 8, 4, 311, device)
    assert not _coarse(plain)
    on, st, off = _both(plain, C[:900], 7, monkeypatch, device, expect_staged=False)
    _check(on, _oracle(plain, vt, C[:900]), 7)


def test_one_workspace_across_call_kinds(device, monkeypatch, prune):
    """A staged top-k, an unstaged top-k, a staged acquire and a top-k on a side stream on one workspace: each
    result is right and acquire_stats describes the call before it."""
    import torch
    pair, vt, C, is_far, ora = prune
    nc = len(C)
    Cd = torch.from_numpy(C).to(device)
    ws = torch.empty(pair.topk_workspace_bytes(nc, 64), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "2")
    _check(pair.acquire_topk(Cd, 64, workspace=ws), ora, 64)
    st = pair.acquire_stats(ws, nc)
    assert st["staged"] and st["evaluated"] <= nc - N_FAR, st
    monkeypatch.setenv("HBX_STAGED", "0")
    _check(pair.acquire_topk(Cd, 64, workspace=ws), ora, 64)
    st0 = pair.acquire_stats(ws, nc)
    assert not st0["staged"] and (st0["seeds"], st0["survivors"], st0["evaluated"]) == (0, 0, nc), st0
    monkeypatch.setenv("HBX_STAGED", "2")
    one = pair.acquire(Cd, workspace=ws)
    st1 = pair.acquire_stats(ws, nc)
    assert one.index == int(ora[3][0]) and st1["staged"] and st1["evaluated"] < nc, st1
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    _check(pair.acquire_topk(Cd, 7, stream=side, workspace=ws), ora, 7)
    st2 = pair.acquire_stats(ws, nc)
    assert st2["staged"] and st2["seeds"] >= 8 and st2["evaluated"] <= nc - N_FAR, st2


@pytest.mark.parametrize("sampler", ["host", "gpu"])
def test_generator_proposals(device, monkeypatch, sampler):
    """BOHB.get_config_topk over 8 continuous hyperparameters: the same proposals with HBX_STAGED=2 and =0 from the
    same RNG state and sampler counter."""
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB
    space = CS.ConfigurationSpace(seed=3)
    for i in range(8):
        space.add_hyperparameter(CS.UniformFloatHyperparameter("x%d" % i, lower=-2, upper=3))
    cg = BOHB(space, device=device, random_fraction=0.0, num_samples=600, sampler=sampler, sampler_seed=11)

    class Job(object):
        pass

    rs = np.random.RandomState(3)
    for j in range(60):
        job = Job()
        job.id, job.exception, job.timestamps = (0, 0, j), None, {}
        job.kwargs = {"config": space.sample_configuration().get_dictionary(), "budget": 1.0}
        job.result = {"loss": float(rs.rand()), "info": None}
        cg.new_result(job)
    assert len(cg.kde_models) == 1
    got = []
    for mode in ("2", "0"):
        monkeypatch.setenv("HBX_STAGED", mode)
        np.random.seed(7)
        cg._sample_counter = 0
        got.append(cg.get_config_topk(1.0, 8))
    assert len(got[0]) == 8 and got[0] == got[1]


def test_merge_of_staged_shards(device, monkeypatch, prune):
    """merge_topk over four staged shards (index_base = the shard's first row) equals the whole pool's top-k."""
    import torch
    from hpbandster_amd.distributed import merge_topk, shard_range
    pair, vt, C, is_far, ora = prune
    Cd = torch.from_numpy(C).to(device)
    monkeypatch.setenv("HBX_STAGED", "2")
    k = 64
    parts = []
    for r in range(4):
        lo, hi = shard_range(len(C), r, 4)
        ws = torch.empty(pair.topk_workspace_bytes(hi - lo, k), dtype=torch.uint8, device=device)
        parts.append(pair.acquire_topk(Cd[lo:hi], k, index_base=lo, workspace=ws))
        assert pair.acquire_stats(ws, hi - lo)["staged"]
    merged, whole = merge_topk(parts, k), pair.acquire_topk(Cd, k)
    _check(merged, ora, k)
    for f in FIELDS:
        assert getattr(merged, f).tobytes() == getattr(whole, f).tobytes(), f


def test_size_policy(device, monkeypatch, prune):
    """HBX_STAGED unset: 2049 candidates x 297 observations lie far below the threshold and do not stage."""
    import torch
    pair, vt, C, is_far, ora = prune
    monkeypatch.delenv("HBX_STAGED", raising=False)
    Cd = torch.from_numpy(np.ascontiguousarray(C[:2049])).to(device)
    ws = torch.empty(pair.topk_workspace_bytes(2049, 8), dtype=torch.uint8, device=device)
    top = pair.acquire_topk(Cd, 8, workspace=ws)
    st = pair.acquire_stats(ws, 2049)
    assert not st["staged"] and st["evaluated"] == 2049 and top.count == 8
