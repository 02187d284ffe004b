"""Host reference of the conditional-space rules (hbx_kde_impute_groups, hbx_rows_deactivate), in numpy.

Restated from the rule's text (include/hbx.h, "conditional search spaces"), not from the C++; the Philox block is
tests/sampler_reference.py's.

Imputation.  The good and the bad set of a group are imputed independently, each from its own original rows.  A set
is the ns rows j = 0 .. ns - 1 in split order: good ``order[seg_off[b] + j]``, bad ``order[seg_off[b+1] - n_bad[b] +
j]``.  Row j is copied to view row v; for t = 0, 1, ... while it holds a NaN: d0 = its lowest NaN dim, m = the set
rows whose original value at d0 is not NaN.  m > 0: the donor is the k-th such row in ascending j,
k = min(m - 1, floor(u_a m)), and every NaN dim of the row takes the donor's original value (NaN possibly).  m == 0:
d0 takes the prior, u_b for a continuous dim, min(L - 1, floor(L u_b)) for L levels.  The draws:
r = philox((ctr & 0xFFFFFFFF, ctr >> 32, 0xFFFD0000 + t, stream_id), key seed), ctr = (counter_base + v) mod 2^64,
u_a = ((r[0] << 32 | r[1]) >> 11) + 0.5) 2^-53, u_b the same of (r[2], r[3]).

The view.  Group b's view rows ``view_off[b] .. view_off[b+1]`` are its imputed good rows, then its imputed bad rows;
``order_v`` the identity local positions, ``src_v`` the original local rows, ``counts[b]`` = (entries filled from
donors, entries filled from the prior).  A group is modelled when 0 < n_good <= n and 0 < n_bad <= n; its view length
must be n_good + n_bad, a skipped group's 0 -- anything else is left unwritten with counts -1.

Deactivation.  Conditions (child, parent, allowed set) in the given order: the child becomes NaN when the parent's
entry is NaN or is not an integer level of the allowed set.
"""
import numpy as np

from tests import sampler_reference as SR

IMPUTE_WORD0 = 0xFFFD0000


def u01(hi, lo):
    return ((((int(hi) << 32) | int(lo)) >> 11) + 0.5) * 2.0 ** -53


def draws(seed, ctr, t, stream_id):
    r = SR.blocks(seed, [int(ctr) % (1 << 64)], IMPUTE_WORD0 + t, stream_id)[0]
    return u01(r[0], r[1]), u01(r[2], r[3])


def prior_value(level, u):
    return u if level == 0 else float(min(level - 1, int(np.floor(level * u))))


def impute_set(rows, levels, seed, counter_base, v_first, stream_id, stats=None):
    """``rows`` [ns, D]: the set's original rows in split order; view rows v_first .. v_first + ns - 1.
    Returns (imputed [ns, D], donor_filled, prior_filled); ``stats["depth"]`` (a dict, optional) keeps the largest
    number of iterations a row took."""
    rows = np.asarray(rows, dtype=np.float64)
    ns, D = rows.shape
    valid = ~np.isnan(rows)
    out = rows.copy()
    n_donor = n_prior = 0
    for j in range(ns):
        datum = out[j]
        if not np.isnan(datum).any():
            continue
        t = 0
        while np.isnan(datum).any():
            assert t < D
            nan_dims = np.nonzero(np.isnan(datum))[0]
            d0 = int(nan_dims[0])
            ua, ub = draws(seed, int(counter_base) + v_first + j, t, stream_id)
            cand = np.nonzero(valid[:, d0])[0]
            m = len(cand)
            if m > 0:
                k = min(m - 1, int(np.floor(ua * m)))
                donor = rows[cand[k]]
                datum[nan_dims] = donor[nan_dims]
                n_donor += int((~np.isnan(donor[nan_dims])).sum())
            else:
                datum[d0] = prior_value(int(levels[d0]), ub)
                n_prior += 1
            t += 1
        if stats is not None:
            stats["depth"] = max(stats.get("depth", 0), t)
    return out, n_donor, n_prior


def modelled(n, ng, nb):
    return 0 < ng <= n and 0 < nb <= n


def view_offsets(seg_off, n_good, n_bad):
    lens = [int(g + b) if modelled(int(seg_off[i + 1] - seg_off[i]), int(g), int(b)) else 0
            for i, (g, b) in enumerate(zip(n_good, n_bad))]
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def impute_groups(X, seg_off, order, n_good, n_bad, levels, view_off, Nv, seed, counter_base=0, stream_id=0,
                  fill=None, stats=None):
    """The whole call.  Returns (Xv [Nv, D], order_v, src_v, counts [B, 2], written bool[Nv]); rows no group writes
    keep ``fill`` (Xv), -1 (order_v, src_v)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    B = len(seg_off) - 1
    Xv = np.full((Nv, D), np.nan if fill is None else fill)
    order_v = np.full(Nv, -1, dtype=np.int64)
    src_v = np.full(Nv, -1, dtype=np.int32)
    counts = np.zeros((B, 2), dtype=np.int32)
    written = np.zeros(Nv, dtype=bool)
    for b in range(B):
        s0, n = int(seg_off[b]), int(seg_off[b + 1] - seg_off[b])
        ng, nb = int(n_good[b]), int(n_bad[b])
        v0, v1 = int(view_off[b]), int(view_off[b + 1])
        want = ng + nb if modelled(n, ng, nb) else 0
        if v0 < 0 or v1 > Nv or v1 - v0 != want:
            counts[b] = -1
            continue
        if not want:
            continue
        o = np.asarray(order[s0:s0 + n])
        sets = [(o[:ng], v0), (o[n - nb:], v0 + ng)]
        for rows_of, vb in sets:
            imp, a, p = impute_set(X[s0 + rows_of], levels, seed, counter_base, vb, stream_id, stats)
            ns = len(rows_of)
            Xv[vb:vb + ns] = imp
            order_v[vb:vb + ns] = np.arange(vb - v0, vb - v0 + ns)
            src_v[vb:vb + ns] = rows_of
            written[vb:vb + ns] = True
            counts[b] += (a, p)
    return Xv, order_v, src_v, counts, written


def deactivate(rows, conditions):
    """``conditions``: (child, parent, allowed levels) in topological order; a copy of ``rows`` with the inactive
    entries NaN."""
    out = np.array(rows, dtype=np.float64, copy=True)
    for r in out:
        for c, p, allowed in conditions:
            v = r[p]
            if not np.isfinite(v) or v != np.floor(v) or int(v) not in set(int(a) for a in allowed):
                r[c] = np.nan
    return out
