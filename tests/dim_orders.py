"""Column orders for mixed continuous / categorical spaces (helper, not a test).

The engine takes ``var_type`` as any string of 'c' and 'u'; almost every other test builds "c" * dc + "u" * du, where
continuous slot k is dim k and categorical slot k is dim dc + k.  Here a case is built c-first by the existing
constructors (synthetic.make_observations, test_gpu_rules._pool, test_gpu_groups._groups) and then its columns are
permuted: ``perm[j]`` is the c-first column that lands at position j, so ``Xp = X[:, perm]``.

``PairCase`` is the one case builder test_oracle_dim_order.py (the conditions on the oracle and on the inputs) and
test_gpu_dim_order*.py (the engine) share: host data only, expected values from the C oracle on the permuted data.
"""
import math

import numpy as np

from oracle import c_oracle
from oracle import kde_oracle as O

EPS = 2.0 ** -53


# ---- the orders ----------------------------------------------------------------------------------------------------
def cat_first(dc, du):
    """every 'u', then every 'c'"""
    return np.array(list(range(dc, dc + du)) + list(range(dc)), dtype=np.int64)


def alternate(dc, du):
    """'ucuc...' while both kinds remain, the rest after"""
    out, c, u = [], 0, 0
    while c < dc and u < du:
        out += [dc + u, c]
        c, u = c + 1, u + 1
    return np.array(out + list(range(c, dc)) + list(range(dc + u, dc + du)), dtype=np.int64)


def lone_ends(dc, du):
    """c-first with the first continuous dim moved to position D - 1 and the last categorical dim to position 0:
    continuous slot dc - 1 is dim D - 1, categorical slot 0 is dim 0"""
    D = dc + du
    assert dc >= 1 and du >= 1
    return np.array([D - 1] + list(range(1, dc)) + list(range(dc, D - 1)) + [0], dtype=np.int64)


def random(seed):
    def order(dc, du):
        return np.random.RandomState(seed).permutation(dc + du).astype(np.int64)
    order.__name__ = "random%d" % seed
    return order


def straddle(dc, du):
    """D > 64: both kinds on both sides of dim 64 -- the categorical dims spread over [0, 64) and over [64, D), a
    continuous dim at 65 -- so the second round of a 64-dim ballot sees dims of both kinds"""
    D = dc + du
    assert D > 65 and du >= 2 and dc >= 2
    hi_free = [64] + list(range(D - 1, 65, -1))  # 65 stays continuous
    n_hi = max(1, min(du // 2, len(hi_free)))
    n_lo = du - n_hi
    assert 1 <= n_lo < 64
    cat_pos = sorted(set(int(p) for p in np.linspace(1, 62, n_lo).astype(int)) | set(hi_free[:n_hi]))
    assert len(cat_pos) == du
    perm, c, u = [], 0, 0
    for j in range(D):
        if j in cat_pos:
            perm.append(dc + u)
            u += 1
        else:
            perm.append(c)
            c += 1
    perm = np.array(perm, dtype=np.int64)
    kinds = perm >= dc
    assert kinds[64:].any() and (~kinds[64:]).any() and kinds[:64].any() and (~kinds[:64]).any()
    return perm


ORDERS = {"cat_first": cat_first, "alternate": alternate, "lone_ends": lone_ends, "random": random,
          "straddle": straddle}


def order_perm(order, dc, du):
    """``order``: a name of ORDERS, ("random", seed) or "randomN" -> the permutation of the dc + du c-first columns"""
    if isinstance(order, tuple):
        return random(order[1])(dc, du)
    if order.startswith("random"):
        return random(int(order[6:]))(dc, du)
    return ORDERS[order](dc, du)


def cfirst_vt(dc, du):
    return "c" * dc + "u" * du


def permute(perm, X=None, C=None, vt=None, bw=None, nlev=None, levels=None):
    """One column permutation applied to whatever is given: observation rows X and candidates C ([..., D]),
    var_type string vt, and the per-dim vectors bw, nlev, levels ([..., D]).  Returns a dict of the permuted ones."""
    perm = np.asarray(perm, dtype=np.int64)
    assert sorted(perm.tolist()) == list(range(len(perm)))
    out = {}
    for key, a in (("X", X), ("C", C), ("bw", bw), ("nlev", nlev), ("levels", levels)):
        if a is not None:
            a = np.asarray(a)
            assert a.shape[-1] == len(perm), (key, a.shape)
            out[key] = np.ascontiguousarray(a[..., perm])
    if vt is not None:
        assert len(vt) == len(perm)
        out["vt"] = "".join(vt[p] for p in perm)
    return out


# ---- the bound of the permutation check ------------------------------------------------------------------------------
def pdf_bound(D, dc, n):
    """Relative distance allowed between the exact pdf of one KDE in two column orders, for a KDE whose kernel
    factors are all positive.  The per-dim factors are bit-identical in both orders; what rounds differently is the
    D - 1 multiplications of the row product, the dc - 1 of prod(bw[continuous]), the division, the pairwise sum of n
    positive terms (ceil(log2 n) levels and the leaf), and the division by n: each at most 2^-53 relative in either
    order, hence the factor 2."""
    return 2.0 * (D + dc + math.ceil(math.log2(max(n, 2))) + 4) * EPS


# ---- one single-pair case ------------------------------------------------------------------------------------------
class PairCase(object):
    """One model and one pool, built c-first and permuted by ``order``.  The attributes without suffix are the
    permuted ones (what the engine gets); ``*0`` the c-first ones.  l, g: the C oracle's exact pdfs of the pool.

    spec keys: dc, du, lev (an int or one count per categorical dim), n_obs, n_cand, seed, cat_bw (> 0: categorical
    bandwidths capped there; < 0: set to -cat_bw, a signed pair; None: the rule's), n_far (test_gpu_rules._pool's),
    const_cat (c-first categorical slot whose column holds one level, bandwidth 0 as the rule gives it),
    cat_lin (categorical bandwidths np.linspace(0.2, 0.5) / (0.6, 0.3): the level counts whose rule gives h > 1)."""

    def __init__(self, spec, order):
        from hpbandster_amd import synthetic as S
        from tests.test_gpu_rules import _pool
        dc, du, lev = spec["dc"], spec["du"], spec["lev"]
        n_obs, n_cand, seed = spec["n_obs"], spec["n_cand"], spec["seed"]
        cat_bw, n_far = spec.get("cat_bw"), spec.get("n_far", min(dc, 8))
        self.dc, self.du, self.D, self.spec, self.order = dc, du, dc + du, spec, order
        self.perm = order_perm(order, dc, du)
        vt0 = cfirst_vt(dc, du)
        X0 = S.make_observations(n_obs, dc, du, lev, seed=seed)
        const_cat = spec.get("const_cat")
        if const_cat is not None:
            X0[:, dc + const_cat] = 1.0
        losses = S.make_losses(n_obs, seed=seed + 1)
        self.losses = losses
        self.min_points = dc + du + 1
        self.g_idx, self.b_idx = O.bohb_split(X0, losses, self.min_points)
        with np.errstate(all="ignore"):
            bwg0, bwb0 = O.normal_reference_bw(X0[self.g_idx]), O.normal_reference_bw(X0[self.b_idx])
        cat = np.array([v == "u" for v in vt0])
        if cat_bw is not None:
            bwg0[cat] = np.minimum(bwg0[cat], cat_bw) if cat_bw > 0 else -cat_bw
            bwb0[cat] = np.minimum(bwb0[cat], cat_bw) if cat_bw > 0 else -cat_bw
        if spec.get("cat_lin"):
            bwg0[dc:], bwb0[dc:] = np.linspace(0.2, 0.5, du), np.linspace(0.6, 0.3, du)
        if const_cat is not None:  # the reference's own bandwidth of a one-level column
            bwg0[dc + const_cat] = bwb0[dc + const_cat] = 0.0
        nlg0, nlb0 = O.num_levels(X0[self.g_idx], vt0), O.num_levels(X0[self.b_idx], vt0)
        rs = np.random.RandomState(seed + 2)
        lev_pool = lev if np.isscalar(lev) else int(min(lev))
        C0 = _pool(rs, X0[self.g_idx], n_cand, dc, du, lev_pool, n_far)
        if not np.isscalar(lev):  # every level of every dim in half the rows
            half = rs.rand(n_cand) < 0.5
            for u in range(du):
                C0[half, dc + u] = rs.randint(0, lev[u], size=int(half.sum()))
        if const_cat is not None:  # most candidates on the one level (the others: 0/0, NaN pdfs)
            on = rs.rand(n_cand) < 0.9
            C0[on, dc + const_cat] = 1.0
        self.vt0, self.X0, self.C0 = vt0, X0, np.ascontiguousarray(C0)
        self.bwg0, self.bwb0, self.nlg0, self.nlb0 = bwg0, bwb0, nlg0, nlb0
        p = permute(self.perm, X=X0, C=C0, vt=vt0)
        self.vt, self.X, self.C = p["vt"], p["X"], p["C"]
        self.bwg, self.bwb = permute(self.perm, bw=bwg0)["bw"], permute(self.perm, bw=bwb0)["bw"]
        self.nlg, self.nlb = permute(self.perm, nlev=nlg0)["nlev"], permute(self.perm, nlev=nlb0)["nlev"]
        self.l, self.g = self.pdfs(self.C)
        self._l0 = None

    def pdfs(self, C, cfirst=False):
        """(l, g) of candidates C ([m, D], in this case's column order, or c-first with cfirst=True)"""
        X, vt = (self.X0, self.vt0) if cfirst else (self.X, self.vt)
        bwg, bwb, nlg, nlb = (self.bwg0, self.bwb0, self.nlg0, self.nlb0) if cfirst else \
            (self.bwg, self.bwb, self.nlg, self.nlb)
        with np.errstate(all="ignore"):
            return (c_oracle.kde_pdf(X[self.g_idx], bwg, vt, nlg, C, exact=True),
                    c_oracle.kde_pdf(X[self.b_idx], bwb, vt, nlb, C, exact=True))

    def cfirst_pdfs(self):
        if self._l0 is None:
            self._l0 = self.pdfs(self.C0, cfirst=True)
        return self._l0

    def kdes(self):
        """(data, bw, nlev, data0, bw0, nlev0, oracle pdfs, c-first oracle pdfs) for the good and the bad KDE"""
        l0, g0 = self.cfirst_pdfs()
        return ((self.X[self.g_idx], self.bwg, self.nlg, self.X0[self.g_idx], self.bwg0, self.nlg0, self.l, l0),
                (self.X[self.b_idx], self.bwb, self.nlb, self.X0[self.b_idx], self.bwb0, self.nlb0, self.g, g0))

    def order_sensitive_share(self):
        """share of the candidates (finite pdfs in both orders) whose l or g bits differ between the two orders"""
        l0, g0 = self.cfirst_pdfs()
        fin = np.isfinite(self.l) & np.isfinite(self.g) & (self.l > 0)
        diff = (self.l.view(np.uint64) != l0.view(np.uint64)) | (self.g.view(np.uint64) != g0.view(np.uint64))
        return float((diff & fin).sum()) / max(1, int(fin.sum()))


# name: the spec of PairCase and the orders the GPU tests run it under ("alternate" and one random; "lone_ends" on
# 24c8u; "straddle" past 64 dims).  300-1500 observations, 515 candidates (a ragged last tile).
def _spec(dc, du, lev, n_obs, seed, orders=None, n_cand=515, **kw):
    d = dict(dc=dc, du=du, lev=lev, n_obs=n_obs, n_cand=n_cand, seed=seed,
             orders=orders or ("alternate", "random%d" % (seed + 3)))
    d.update(kw)
    return d


PAIR_SPECS = {
    "3c1u": _spec(3, 1, 4, 1000, 21, cat_bw=0.8, n_far=3, orders=("alternate", "random28")),  # fp32 kernels; "ccuc"
    "6c2u": _spec(6, 2, 4, 300, 11, cat_bw=0.8, n_far=6),                        # h32
    "24c8u": _spec(24, 8, 4, 1500, 1, cat_bw=0.5, orders=("alternate", "random4", "lone_ends")),  # coarse 32x32
    "signed": _spec(8, 4, 4, 300, 31, cat_bw=-1.2),                              # categorical bandwidth 1.2
    "16c8u3": _spec(16, 8, 3, 600, 41, cat_bw=0.8),                              # under every entry of KERNELS
    "oh20": _spec(20, 6, [3, 5, 2, 3, 4, 3], 1500, 51, cat_bw=0.8),              # one-hot, odd level counts
    "oh24": _spec(24, 3, [4, 4, 4], 1500, 53, cat_bw=0.8),                       # one dense f16 one-hot step
    "f32oh12": _spec(12, 16, 3, 300, 71, cat_bw=0.8),                            # f32 one-hot product, kc 4
    "f32valu33": _spec(33, 8, 12, 300, 73, cat_lin=True),                        # f32 VALU matching, dc_pad 64
    "70c4u": _spec(70, 4, 4, 320, 81, cat_bw=0.8, orders=("straddle", "random84")),   # exact-only: past the buckets
    "3c33u": _spec(3, 33, 3, 300, 83, cat_bw=0.8, n_far=3),                      # exact-only
    "const8": _spec(8, 3, 4, 300, 91, cat_bw=0.8, const_cat=1),                  # a one-level dim between two active
    "const24": _spec(24, 3, 4, 600, 93, cat_bw=0.8, const_cat=1),
    "8c8u4": _spec(8, 8, 4, 600, 95, cat_bw=0.8),                                # ln-pdf: 8 categorical slots
    "staged": _spec(24, 8, 4, 1000, 97, cat_bw=0.5, n_cand=4099),                # enough candidates for the stages
    "split": _spec(24, 8, 4, 10000, 99, cat_bw=0.5, n_cand=64),                  # observation ranges per block
}

_PAIR_CASES = {}


def pair_case(name, order):
    key = (name, order)
    if key not in _PAIR_CASES:
        _PAIR_CASES[key] = PairCase(PAIR_SPECS[name], order)
    return _PAIR_CASES[key]


def pair_case_ids():
    return [(name, order) for name in sorted(PAIR_SPECS) for order in PAIR_SPECS[name]["orders"]]


# ---- the grouped cases ---------------------------------------------------------------------------------------------
# one shape per slot bucket and pair loop of the grouped kernels; past 64 dims also under "straddle"
GROUP_SHAPES = [(5, 2), (12, 3), (3, 10), (24, 8), (40, 6), (60, 8), (70, 4)]
GROUP_B, GROUP_C, GROUP_S, GROUP_K = 6, 65, 3, 5


def group_case_ids():
    out = []
    for dc, du in GROUP_SHAPES:
        orders = ("alternate", "random%d" % (dc + du)) + (("straddle",) if dc + du > 64 else ())
        out += [(dc, du, o) for o in orders]
    return out


def group_split(losses, D):
    """bohb.py:220-237 for one group: numpy 1.26.4's argsort of the losses, the integer floor sizes clipped to n (a
    slice), no model where a set has no more rows than dims."""
    from oracle import np_argsort
    n = len(losses)
    ng, nb = O.bohb_split_sizes(n, D + 1)
    ng, nb = min(ng, n), min(nb, n)
    if ng <= D or nb <= D:
        return None
    idx = np_argsort.argsort(losses)
    return idx[:ng], idx[n - nb:]


class GroupCase(object):
    """The first GROUP_B groups of test_gpu_groups._groups (no model, a constant continuous column, one observed
    level, signed, unsupported codes, a plain one), S pools of C candidates each, permuted by ``order`` after
    construction.  Per group with a model: the oracle's split, bandwidths, level counts and exact pdfs."""

    def __init__(self, dc, du, order, min_bandwidth=None):
        from tests.test_gpu_groups import _groups
        B, C, S = GROUP_B, GROUP_C, GROUP_S
        self.dc, self.du, self.D, self.B, self.order = dc, du, dc + du, B, order
        X0, losses, seg, vt0, levels, cands0, kinds = _groups(dc, du, C * S, B=11)
        seg = seg[:B + 1]
        n = int(seg[-1])
        self.seg, self.losses = seg, np.ascontiguousarray(losses[:n])
        self.kinds = {b: k for b, k in kinds.items() if b < B and k != "dup"}
        self.perm = order_perm(order, dc, du)
        lv0 = np.array([0] * dc + [int(v) for v in levels], dtype=np.int32)
        p = permute(self.perm, X=X0[:n], C=cands0[:B], vt=vt0, levels=lv0)
        self.vt0, self.vt, self.X0, self.X = vt0, p["vt"], np.ascontiguousarray(X0[:n]), p["X"]
        self.cands0 = np.ascontiguousarray(cands0[:B]).reshape(B, S, C, self.D)
        self.cands = p["C"].reshape(B, S, C, self.D)
        self.levels = p["levels"]
        self.rows, self.bw, self.nlev, self.pdf, self.pdf0 = {}, {}, {}, {}, {}
        for b in range(B):
            sp = group_split(self.losses[seg[b]:seg[b + 1]], self.D)
            if sp is None:
                continue
            self.rows[b] = sp
            Xb = self.X[seg[b]:seg[b + 1]]
            with np.errstate(all="ignore"):
                bws = [O.normal_reference_bw(Xb[r]) for r in sp]
            if min_bandwidth:
                bws = [np.where(h < min_bandwidth, min_bandwidth, h) for h in bws]
            self.bw[b] = bws
            self.nlev[b] = [O.num_levels(Xb[r], self.vt) for r in sp]
            if self.kinds.get(b) != "unsupported":
                self.pdf[b] = self._pdfs(b, self.X, self.vt, self.cands[b], np.arange(self.D))
        self.min_bandwidth = min_bandwidth

    def _pdfs(self, b, X, vt, cands, inv):
        seg = self.seg
        Xb = X[seg[b]:seg[b + 1]]
        out = []
        with np.errstate(all="ignore"):
            for r, bw, nl in zip(self.rows[b], self.bw[b], self.nlev[b]):
                out.append(c_oracle.kde_pdf(Xb[r], bw[inv], vt, nl[inv], cands.reshape(-1, self.D), exact=True)
                           .reshape(cands.shape[:-1]))
        return out

    def cfirst_pdfs(self, b):
        """the same group's pdfs with every column back in c-first order"""
        if b not in self.pdf0:
            inv = np.argsort(self.perm)  # c-first column c sits at permuted position inv[c]
            self.pdf0[b] = self._pdfs(b, self.X0, self.vt0, self.cands0[b], inv)
        return self.pdf0[b]

    def pdfs_of(self, b, pts):
        """(l, g) of points pts [m, D] in this case's column order under group b's model"""
        return self._pdfs(b, self.X, self.vt, np.asarray(pts), np.arange(self.D))


_GROUP_CASES = {}


def group_case(dc, du, order):
    key = (dc, du, order)
    if key not in _GROUP_CASES:
        _GROUP_CASES[key] = GroupCase(dc, du, order)
    return _GROUP_CASES[key]


# ---- the cross-validation cases --------------------------------------------------------------------------------------
CV_LAYOUTS = ["ucu", "cuuc", "".join("uc"[i % 2] for i in range(12))]


def cv_case(vt, n=40, seed=17):
    """n rows in layout vt (built c-first and permuted to it), 3 levels per categorical dim, and two bandwidth
    points below 1 in every categorical dim.  Returns (X, bw_points, X0, vt0, perm)."""
    dc, du = vt.count("c"), vt.count("u")
    rs = np.random.RandomState(seed + len(vt))
    X0 = np.column_stack([rs.rand(n, dc), rs.randint(0, 3, (n, du))]).astype(np.float64)
    ci, ui = [i for i, t in enumerate(vt) if t == "c"], [i for i, t in enumerate(vt) if t == "u"]
    perm = np.empty(len(vt), dtype=np.int64)
    perm[ci], perm[ui] = np.arange(dc), dc + np.arange(du)
    vt0 = cfirst_vt(dc, du)
    assert permute(perm, vt=vt0)["vt"] == vt
    h0 = O.normal_reference_bw(X0)
    h0[dc:] = np.minimum(h0[dc:], 0.8)
    pts0 = np.stack([h0, h0 * np.where(np.arange(dc + du) < dc, 0.6, 0.5) + 0.01 * rs.rand(dc + du)])
    return permute(perm, X=X0)["X"], permute(perm, bw=pts0)["bw"], X0, vt0, perm
