"""BOHB's candidate draws on the host (bohb.py:133-147), bit for bit the reference's: the raw MT19937 state of a
legacy ``RandomState`` (``_MT``), the draws made on it in one native call (``hbx_bohb_draw``) with scipy's
truncnorm inversion restated over cached per-row terms (``_draw_fast``), and the reference's element-by-element
path (``_draw_rvs``) that runs wherever a once-per-process check finds numpy or scipy not as assumed.
config_generators/bohb.py draws through these; nothing here knows about configuration spaces or models on the GPU.
"""

import ctypes
import logging

import numpy as np
import scipy.stats as sps

from . import _native


def _once(memo, check, warning):
    """A once-per-process check: ``memo[0]``, on first use set to whether ``check()`` holds -- False, never
    raising, when it raises -- with ``warning`` logged once when it does not hold."""
    if memo[0] is None:
        try:
            memo[0] = bool(check())
        except Exception:
            memo[0] = False
        if not memo[0]:
            logging.getLogger('hpbandster').warning(warning)
    return memo[0]


class _MT(object):
    """The raw MT19937 state (key[624] words + position: 2500 bytes) of a legacy ``RandomState`` -- a
    snapshot, compare or restore in ~1 us, where ``get_state`` / ``set_state`` cost ~60 us each (they
    build and parse the state tuple).  The Gaussian cache of the legacy generator is not part of it:
    BOHB's draws (``rand``, ``randint``, scipy's truncnorm by inversion of a uniform) never touch it.
    The layout is numpy's ``mt19937_state``; ``mt_layout_ok()`` checks it against ``get_state`` /
    ``set_state`` once per process before anything relies on it."""
    NB = 624 * 4 + 4

    def __init__(self, rs):
        bg = rs._bit_generator
        if type(bg).__name__ != "MT19937":
            raise TypeError("not an MT19937 RandomState")
        self.rs, self.addr, self.lock = rs, bg.ctypes.state_address, bg.lock

    def snap(self):
        return ctypes.string_at(self.addr, self.NB)

    def load(self, raw):
        ctypes.memmove(self.addr, raw, self.NB)


_LAYOUT = [None]


def _mt_layout_check():
    a, b = np.random.RandomState(20240917), np.random.RandomState(77)
    a.random_sample(700)  # position off the block boundary
    ma, mb = _MT(a), _MT(b)
    st = a.get_state(legacy=True)
    ok = ma.snap() == np.asarray(st[1], dtype="<u4").tobytes() + np.int32(st[2]).tobytes()
    mb.load(ma.snap())
    sb = b.get_state(legacy=True)
    ok = ok and np.array_equal(sb[1], st[1]) and sb[2] == st[2]
    return ok and np.array_equal(a.random_sample(3), b.random_sample(3))


def mt_layout_ok():
    """Once per process: the raw bytes at the bit generator's state address are get_state()'s key words
    and position, and load() of another state's bytes gives that state's get_state() (and its next
    draws).  False (never raising) when numpy's layout is not the one assumed: the raw-state users then
    step aside -- speculative batches are not made, the host draws take scipy's per-element path."""
    return _once(_LAYOUT, _mt_layout_check,
                 "numpy's MT19937 state layout is not the assumed one: speculative batches and the fast host draws "
                 "are off (results unchanged)")


_GLOBAL = [None]


def _global_mt():
    """_MT of numpy's global RandomState (the one np.random.rand / randint / scipy's rvs draw from), or
    None when its raw state cannot be used."""
    R = np.random.mtrand._rand
    g = _GLOBAL[0]
    if g is None or g.rs is not R:
        if not mt_layout_ok():
            return None
        try:
            g = _GLOBAL[0] = _MT(R)
        except (TypeError, AttributeError):
            return None
    return g


_HOSTDRAW = [None]  # (the benchmark sets entry 0 to False to time the per-element path)


def _host_draw_check():
    if not (mt_layout_ok() and int(_native.lib().hbx_mt_state_bytes()) == _MT.NB):
        return False
    L = _native.lib()
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    ma = _MT(a)
    out = np.empty(1500)
    _native.check(L.hbx_mt_draw(ma.addr, 0, out.size, 0, out.ctypes.data))
    ok = np.array_equal(out, b.random_sample(out.size))
    for high in (1, 2, 3, 4, 7, 100, 1000, 65537, 2 ** 31 + 5):
        o = np.empty(64)
        _native.check(L.hbx_mt_draw(ma.addr, 1, o.size, high, o.ctypes.data))
        ok = ok and np.array_equal(o, [b.randint(0, high) for _ in range(o.size)])
    if not (ok and ma.snap() == _MT(b).snap()):
        return False
    rs = np.random.RandomState(11)
    data = np.column_stack([rs.rand(9, 3), rs.randint(0, 3, (9, 2))]).astype(np.float64)
    data[4, 0], data[2, 1] = 0.0, 1.0
    kde = _HostModel(data, np.array([0.2, 0.05, 0.6, 0.4, 0.9]))
    lv = np.array([0, 0, 0, 3, 4])
    a, b = np.random.RandomState(6), np.random.RandomState(6)
    fast = _draw_fast(kde, lv, 3, 16, a, _MT(a))
    slow = _draw_rvs(kde, lv, 3, 16, b)
    return np.array_equal(fast, slow) and _MT(a).snap() == _MT(b).snap()


def host_draw_ok():
    """Once per process: hbx_bohb_draw (libhbx's restatement of the draws, on numpy's own state) agrees with
    numpy and scipy -- random_sample and randint streams, and a small get_config draw against the
    per-element scipy path, values and final state bit for bit.  False (never raising) otherwise: the
    per-element path then runs."""
    return _once(_HOSTDRAW, _host_draw_check,
                 "hbx_bohb_draw disagrees with numpy/scipy here: BOHB draws candidates element by element")


class _HostModel(object):
    """The two fields of a KDE the draws read (``data`` rows and ``bw``)."""

    def __init__(self, data, bw):
        self.data, self.bw = data, bw


def _draw_rvs(kde_good, levels, bw_factor, num_samples, R):
    """bohb.py:133-147 element by element: R.randint for the datum, one scipy truncnorm.rvs per continuous
    dim (bounds from bw, scale bw_factor * bw), keep-or-resample per categorical dim."""
    D = len(levels)
    cands = np.empty((num_samples, D), dtype=np.float64)
    data = kde_good.data
    bws = kde_good.bw
    for i in range(num_samples):
        idx = R.randint(0, len(data))
        for d, (m, bw, t) in enumerate(zip(data[idx], bws, levels)):
            if t == 0:
                cands[i, d] = sps.truncnorm.rvs(-m / bw, (1 - m) / bw, loc=m, scale=bw_factor * bw, random_state=R)
            else:
                if R.rand() < (1 - bw):
                    cands[i, d] = m
                else:
                    cands[i, d] = R.randint(t)
    return cands


class _TruncnormTerms(object):
    """The uniform-independent terms of scipy's ``truncnorm._ppf`` for one KDE's observation rows, filled
    row by row as draws first pick them (a model serves every call until the next refit, and BOHB's datum is
    one of its good rows: after a call or two every row is in).  Per (row, continuous dim), with a = -m/bw,
    b = (1 - m)/bw (scipy 1.15 ``_continuous_distns.py``, ``truncnorm_gen._ppf`` / ``_log_gauss_mass``):
    ``lp`` = log_ndtr(a) where a < 0 (``ppf_left``), log_ndtr(-b) otherwise (``ppf_right``); ``mass`` =
    log1p(-ndtr(a) - ndtr(-b)), the central case of ``_log_gauss_mass``; ``ok`` False where that case does not
    apply (b <= 0: a datum at the upper bound, a > 0, non-finite bounds) -- those elements take scipy's own
    ``_ppf``."""

    def __init__(self, data, bw):
        self.data, self.bw = data, bw
        n, D = data.shape
        self.lp = np.empty((n, D))
        self.mass = np.empty((n, D))
        self.left = np.zeros((n, D), dtype=np.bool_)
        self.ok = np.zeros((n, D), dtype=np.bool_)
        self.have = np.zeros(n, dtype=np.bool_)

    def fill(self, rows, cont):
        import scipy.special as sc
        r = np.unique(rows[~self.have[rows]])
        if r.size:
            m = self.data[np.ix_(r, cont)]
            h = self.bw[cont]
            with np.errstate(all="ignore"):  # (a zero bandwidth: no inversion is asked for that dim)
                a, b = -m / h, (1 - m) / h
                left = a < 0
                self.lp[np.ix_(r, cont)] = sc.log_ndtr(np.where(left, a, -b))
                self.mass[np.ix_(r, cont)] = sc.log1p(-sc.ndtr(a) - sc.ndtr(-b))
            self.left[np.ix_(r, cont)] = left
            self.ok[np.ix_(r, cont)] = (b > 0) & (a <= 0) & np.isfinite(a) & np.isfinite(b)
            self.have[r] = True


def _ppf_from_terms(q, lp, mass, left):
    """scipy's truncnorm._ppf at uniforms q from the terms above, the same numpy / scipy.special ufuncs in the
    same order: log_Phi_x = logsumexp([lp, log(q) + mass]) (log1p(-q) on the right), scipy 1.15's
    ``_logsumexp`` for two real rows (the larger one taken out of the sum: (log1p(exp(lo - hi)) + log(m)) + hi,
    m the number of rows equal to the larger), then ndtri_exp (negated on the right).  Formed here as
    log1p(exp(min - max)) + max: for m = 1, log(m) = 0 adds nothing to log1p(.) >= 0; for m = 2 (the rows
    equal), exp(0) = 1 and log1p(1) is log(2) (checked by ppf_terms_ok), where scipy adds log(2) to log1p(0) = 0.
    Elementwise, so a subset gives the values the whole array would.  Non-finite log_Phi_x inputs come back as
    ``bad`` positions for scipy's own _ppf."""
    import scipy.special as sc
    with np.errstate(all="ignore"):
        x = np.where(left, np.log(q), np.log1p(-q))
        x += mass
        hi = np.maximum(lp, x)
        s = np.minimum(lp, x)
        s -= hi
        np.exp(s, out=s)
        np.log1p(s, out=s)
        s += hi
        y = sc.ndtri_exp(s)
    np.negative(y, out=y, where=~left)
    return y, ~np.isfinite(hi)


_PPF = [None]


def _ppf_terms_check():
    rs = np.random.RandomState(17)
    nr, nd = 200, 20
    m = rs.rand(nr, nd)
    m[:4] = 0.0
    m[4:6] = 1.0
    m[6:10] = rs.choice([1e-12, 1 - 1e-12, 1e-300, 0.5], (4, nd))
    h = np.exp(rs.uniform(np.log(1e-4), np.log(5.0), nd))
    q = rs.rand(nr, nd)
    q[10:12] = 0.0
    q[12:16] = rs.choice([1e-300, 1e-17, 1 - 2 ** -53, 0.5], (4, nd))
    t = _TruncnormTerms(m, h)
    t.fill(np.arange(nr), np.arange(nd))
    with np.errstate(all="ignore"):
        ref = sps.truncnorm._ppf(q, -m / h, (1 - m) / h)
    y, bad = _ppf_from_terms(q, t.lp, t.mass, t.left)
    use = t.ok & ~bad
    ok = bool(use.sum() > nr * nd - 3 * nd) and np.array_equal(y[use].view(np.uint64), ref[use].view(np.uint64))
    one = np.ones(4)  # the equal-rows case of the logsumexp (_ppf_from_terms)
    return ok and np.array_equal(np.log1p(one).view(np.uint64), np.log(one + one).view(np.uint64))


def ppf_terms_ok():
    """Once per process: _ppf_from_terms equals scipy's own truncnorm._ppf bit for bit over BOHB's range and its
    edges (uniforms 0, tiny, near 1; a datum at 0 (a = -0: the right case), at 1 (b = 0: scipy's path), near the
    bounds; narrow and wide bandwidths).  False (never raising) otherwise: the draws then invert through scipy's
    _ppf, as before."""
    return _once(_PPF, _ppf_terms_check,
                 "the truncnorm inversion terms disagree with scipy's truncnorm._ppf here: BOHB inverts through scipy")


def _draw_fast(kde_good, levels, bw_factor, num_samples, R, mt, out=None):
    """The same draws in one native call on R's own MT19937 state (hbx_bohb_draw, the reference's
    consumption order), then the truncnorm inversion of the call's uniforms and rvs's ``* scale + loc`` --
    the arithmetic rvs applies to each uniform, elementwise, so the values are the per-element path's bit for
    bit (checked by host_draw_ok and tests/test_host_draw.py).  The inversion reuses the model's per-row terms
    (``_TruncnormTerms``; scipy's own ``truncnorm._ppf`` when ppf_terms_ok() fails and for the elements the
    terms do not cover).  A domain error raises ValueError with R left where scipy's raise leaves it."""
    data = kde_good.data
    if not (isinstance(data, np.ndarray) and data.dtype == np.float64 and data.flags.c_contiguous):
        data = np.ascontiguousarray(data, dtype=np.float64)
    bws = np.ascontiguousarray(kde_good.bw, dtype=np.float64)
    lv = np.ascontiguousarray(levels, dtype=np.int64)
    n, D = data.shape
    vals = np.empty((num_samples, D)) if out is None else out
    if not vals.flags.c_contiguous:
        raise ValueError("_draw_fast: out must be C-contiguous")
    cap = num_samples * D
    uni = np.empty(cap)
    comp = np.empty(2 * cap, dtype=np.int64)
    datum = np.empty(num_samples, dtype=np.int64)
    stop = ctypes.c_int64(-1)
    nc = ctypes.c_int64(0)
    with mt.lock:
        rc = _native.lib().hbx_bohb_draw(mt.addr, data.ctypes.data, n, D, bws.ctypes.data, lv.ctypes.data,
                                         float(bw_factor), num_samples, vals.ctypes.data, uni.ctypes.data, None,
                                         datum.ctypes.data, ctypes.addressof(stop), comp.ctypes.data,
                                         ctypes.addressof(nc))
    if rc == 1:
        raise ValueError("Domain error in arguments (truncnorm bounds of candidate %d, dim %d; bohb.py:141)"
                         % divmod(stop.value, D))
    _native.check(rc)
    k = nc.value
    if k == 0:
        return vals
    # the elements to invert, in draw order: uniform q, element index e, term index ti = datum D + dim
    q, e, ti = uni[:k], comp[:k], comp[cap:cap + k]
    flat = vals.reshape(-1)
    loc = flat.take(e)
    h = bws.take(ti % D)
    if ppf_terms_ok():
        t = getattr(kde_good, "_tn_terms", None)
        if t is None or t.data is not data or t.bw is not bws or t.lp.shape != (n, D):
            t = _TruncnormTerms(data, bws)
            try:
                kde_good._tn_terms = t
            except AttributeError:  # (an object that takes no attributes: terms for this call only)
                pass
        t.fill(datum, np.flatnonzero(lv == 0))
        y, bad = _ppf_from_terms(q, t.lp.reshape(-1).take(ti), t.mass.reshape(-1).take(ti),
                                 t.left.reshape(-1).take(ti))
        rest = bad | ~t.ok.reshape(-1).take(ti)
        if rest.any():
            y[rest] = sps.truncnorm._ppf(q[rest], -loc[rest] / h[rest], (1 - loc[rest]) / h[rest])
    else:
        y = sps.truncnorm._ppf(q, -loc / h, (1 - loc) / h)
    flat[e] = y * (bw_factor * h) + loc
    return vals
