"""The cases of the imputation tests (tests/test_impute_host.py, tests/test_gpu_impute.py) and their numpy reference
results (tests/impute_reference.py), computed once per case and shared.

Shapes: D in {1, 5, 33, 70} with the kinds interleaved (tests/dim_orders.py), B in {1, 3, 40}; set sizes 1, 31, 32,
33 and 100 (mask-word boundaries), a group with n_good + n_bad > n, skipped and empty groups between modelled ones.
NaN patterns, one per group in turn: a column NaN in the whole group (continuous and categorical: the prior), a
column with exactly one non-NaN row, a row NaN in every dim, NaN in dim 0 only, a forced donor chain of depth 3,
+-inf entries, no NaN at all, 30 % NaN in a third of the dims.  "big": 256 dims x 4096 rows per set, which the LDS
masks cannot hold."""
import numpy as np

from tests import dim_orders as DO
from tests import impute_reference as IR

# (n, n_good, n_bad)
GROUPS = [(40, 1, 33), (63, 31, 32), (130, 33, 100), (50, 32, 31), (20, 0, 0), (0, 0, 0), (10, 11, 3), (100, 100, 1)]
PATTERNS = ["all_nan_cols", "one_valid", "nan_row", "dim0_only", "chain", "inf", "clean", "random"]


def levels_of(D, seed):
    """D level counts, 0 = continuous, kinds interleaved"""
    du = D // 3 if D > 1 else seed % 2
    dc = D - du
    lv = np.array([0] * dc + [2 + (i + seed) % 4 for i in range(du)], dtype=np.int32)
    if dc and du:
        lv = lv[DO.alternate(dc, du)]
    return np.ascontiguousarray(lv)


def _inject(rs, Xg, o, ng, levels, pattern):
    n, D = Xg.shape
    cont = [d for d in range(D) if levels[d] == 0]
    cat = [d for d in range(D) if levels[d] > 0]
    if pattern == "clean" or n == 0:
        return
    if pattern != "chain":  # a light background of single NaN entries (the chain's donors are forced: none there)
        Xg[rs.rand(n, D) < 0.05] = np.nan
    if pattern == "all_nan_cols":
        for dims in (cont, cat):
            if dims:
                Xg[:, dims[len(dims) // 2]] = np.nan
    elif pattern == "one_valid":
        d = D // 2
        keep = Xg[o[0], d] if not np.isnan(Xg[o[0], d]) else 1.0
        Xg[:, d] = np.nan
        Xg[o[0], d] = keep  # the good set's first row; the bad set has it only where the sets overlap
    elif pattern == "nan_row":
        Xg[o[0]] = np.nan
        Xg[o[n - 1]] = np.nan
    elif pattern == "dim0_only":
        Xg[o[::3], 0] = np.nan
    elif pattern == "chain" and D >= 3 and ng >= 4:
        keep = Xg[o[:3], :3].copy()
        Xg[:, :3] = np.nan  # dims 0, 1, 2 hold a value in rows o[0], o[1], o[2] only, one dim each
        for i in range(3):
            Xg[o[i], i] = keep[i, i]
    elif pattern == "inf":
        for d in cont:  # (continuous columns only: a categorical entry stays a level)
            Xg[rs.rand(n) < 0.08, d] = np.inf
            Xg[rs.rand(n) < 0.08, d] = -np.inf
    elif pattern == "random":
        dims = rs.permutation(D)[:max(1, D // 3)]
        for d in dims:
            Xg[rs.rand(n) < 0.3, d] = np.nan


class Case(object):
    def __init__(self, name, D, groups, seed, counter_base=0, stream_id=0, patterns=None, sparse=None):
        rs = np.random.RandomState(seed)
        self.name, self.D, self.B = name, D, len(groups)
        self.levels = levels_of(D, seed)
        self.seg_off = np.concatenate(([0], np.cumsum([g[0] for g in groups]))).astype(np.int64)
        self.n_good = np.array([g[1] for g in groups], dtype=np.int64)
        self.n_bad = np.array([g[2] for g in groups], dtype=np.int64)
        N = int(self.seg_off[-1])
        X = rs.rand(max(N, 1), D)
        for d in range(D):
            if self.levels[d]:
                X[:, d] = rs.randint(0, self.levels[d], size=X.shape[0])
        self.order = np.zeros(max(N, 1), dtype=np.int64)
        self.patterns = []
        for b, (n, ng, nb) in enumerate(groups):
            s0 = int(self.seg_off[b])
            o = rs.permutation(n).astype(np.int64)
            self.order[s0:s0 + n] = o
            pat = (patterns or PATTERNS)[(b + seed) % len(patterns or PATTERNS)]
            self.patterns.append(pat)
            if sparse is None:
                _inject(rs, X[s0:s0 + n], o, ng, self.levels, pat)
            else:  # few rows with NaN, some of them deep
                rows = rs.permutation(n)[:int(n * sparse)]
                for r in rows:
                    X[s0 + r, rs.rand(D) < rs.choice([0.02, 0.5])] = np.nan
                X[s0:s0 + n, 7] = np.nan  # one column for the prior
        self.X = np.ascontiguousarray(X)
        self.view_off = IR.view_offsets(self.seg_off, self.n_good, self.n_bad)
        self.Nv = int(self.view_off[-1])
        self.seed, self.counter_base, self.stream_id = 0x1234567 + seed, counter_base, stream_id
        self._ref, self.stats = None, {}

    def reference(self):
        if self._ref is None:
            self._ref = IR.impute_groups(self.X, self.seg_off, self.order, self.n_good, self.n_bad, self.levels,
                                         self.view_off, self.Nv, self.seed, self.counter_base, self.stream_id,
                                         stats=self.stats)
        return self._ref


def _groups_for(B):
    if B == 1:
        return [GROUPS[2]]
    if B == 3:
        return [GROUPS[0], GROUPS[4], GROUPS[3]]
    return [GROUPS[i % len(GROUPS)] for i in range(B)]


CASE_IDS = ["D%d-B%d" % (D, B) for D in (1, 5, 33, 70) for B in (1, 3, 40)] + ["chain-B1", "big"]
_CASES = {}


def case(name):
    if name not in _CASES:
        if name == "big":
            c = Case(name, 256, [(4096, 4096, 4096)], 5, counter_base=(1 << 32) - 1000, sparse=0.04)
        elif name == "chain-B1":
            c = Case(name, 5, [GROUPS[2]], 9, patterns=["chain"])
        else:
            D, B = (int(v[1:]) for v in name.split("-"))
            # every third case counts across the low word's end, one across 2^64
            cb = {0: 0, 1: (1 << 32) - 7, 2: (1 << 64) - 11}[(D + B) % 3]
            c = Case(name, D, _groups_for(B), D * 100 + B, counter_base=cb, stream_id=(D + B) % 5)
        _CASES[name] = c
    return _CASES[name]
