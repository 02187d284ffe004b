"""Host reference of the GPU candidate sampler (hbx_kde_sample, hbx_kde_sample_groups): every draw, in fp64.

Restated from the file header of hbx_sample.hip in numpy / scipy, not from the kernel's loop.

The stream.  Candidate i of a call draws from the Philox4x32-10 counter
    (ctr & 0xFFFFFFFF, ctr >> 32, word, stream_id),  ctr = (counter_base + i) mod 2^64,
under the key (seed & 0xFFFFFFFF, seed >> 32).  A block r is four 32-bit words.
* Datum: word 0xFFFFFFFF, bits = r[0] << 32 | r[1], idx = (bits * n) >> 64 (exact integers).
* Dim d: word(d) = (d // 2) % 4 + 4 * (d // 16), slot(d) = 2 * ((d // 8) % 2) + d % 2, u = (r[slot] + 0.5) 2^-32.
  That is the closed form of "4 lanes per candidate, lane g takes the pairs g, g + 4, ..., a new block every second
  pair": pair k = d // 2 belongs to lane g = k % 4 as its q-th pair, q = k // 4, word = g + 4 (q // 2),
  slot = 2 (q % 2) + d % 2.  The 4 is part of the stream's definition.  The map has period 16 in d: dims d and
  d + 16 use the same slot of words 4 apart, each word serves exactly 4 dims, and d -> (word, slot) is one-to-one
  for every d.  With D <= 256 the words stay below 64, far from the reserved words from 0xFFFE0000 up.

The rule per dim of the datum row m, bandwidth h (bohb.py:133-147):
* categorical (levels[d] = t > 0): thr = 1 - h; u < thr keeps m; else v = (u - thr) * (1 / h) (v = u when
  thr <= 0) and the level is min(int(v * t), t - 1).  Plain IEEE double operations, so the level is exact.
* continuous: a = -m * (1 / h), b = (1 - m) * (1 / h); not (a < b) is a domain error (NaN, error byte 1, the
  candidate's other dims still drawn).  a > 0 is mirrored (z drawn from [-b, -a], x = m - s z).
  p = Phi(lo) + u (Phi(hi) - Phi(lo)), z = Phi^-1(p) on the smaller tail, clamped to [lo, hi],
  x = m + bw_factor * h * (+-z).
"""
import numpy as np
from scipy.special import ndtr, ndtri

MASK32 = np.uint64(0xFFFFFFFF)
DATUM_WORD = 0xFFFFFFFF
RESERVED_WORD0 = 0xFFFE0000  # the words from here up belong to other draws (hbx_philox.h)
LANES = 4                    # lanes per candidate: part of the stream's definition
EDGE = 2.0 ** -40            # a categorical draw this close to a decision edge may be left out of a comparison


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays: counter [..., 4], key [..., 2] -> uint32 [..., 4]."""
    c = np.asarray(counter).astype(np.uint64) & MASK32
    k = np.asarray(key).astype(np.uint64) & MASK32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bit: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + w0) & MASK32, (k1 + w1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def candidate_counters(counter_base, count):
    """ctr of candidates 0..count-1 as Python ints: (counter_base + i) mod 2^64"""
    return [(int(counter_base) + i) % (1 << 64) for i in range(int(count))]


def blocks(seed, ctrs, word, stream_id):
    """The Philox block of every candidate counter in ``ctrs`` at ``word``: uint32 [len(ctrs), 4]"""
    seed = int(seed) % (1 << 64)
    counter = np.array([[c & 0xFFFFFFFF, c >> 32, int(word), int(stream_id)] for c in ctrs], dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(counter.reshape(-1, 4), np.broadcast_to(key, (len(ctrs), 2)))


def datum_index(seed, ctrs, stream_id, n):
    r = blocks(seed, ctrs, DATUM_WORD, stream_id)
    return np.array([(((int(a) << 32) | int(b)) * int(n)) >> 64 for a, b in zip(r[:, 0], r[:, 1])], dtype=np.int64)


def dim_word_slot(d):
    """(word, slot) of dim d"""
    k = d // 2
    g, q = k % LANES, k // LANES
    return g + LANES * (q // 2), 2 * (q % 2) + (d % 2)


def uniforms(seed, ctrs, stream_id, D):
    """u [len(ctrs), D]: the uniform of every dim of every candidate"""
    ws = [dim_word_slot(d) for d in range(D)]
    blk = {w: blocks(seed, ctrs, w, stream_id) for w in sorted(set(w for w, _ in ws))}
    u = np.empty((len(ctrs), D))
    for d, (w, s) in enumerate(ws):
        u[:, d] = (blk[w][:, s].astype(np.float64) + 0.5) * 2.0 ** -32
    return u


class Draws(object):
    """What the reference knows about a call's draws.  Per candidate: ``datum`` int64 [Nc], ``err`` uint8 [Nc].
    Per (candidate, dim), [Nc, D]: ``cands`` (x), ``u``, ``m`` (the datum's value), ``domain`` (domain error);
    continuous dims: ``zs`` (the clamped standard draw with the mirror's sign applied: x = m + bw_factor h zs),
    ``lo`` / ``hi`` (the bounds of zs), ``ptail`` = min(p, 1 - p), ``clamped`` (zs sits on a bound);
    categorical dims: ``near_edge`` (within EDGE of a decision edge).  NaN / False where a field does not apply."""


def draw(m, h, levels, bw_factor, u):
    """The rule applied to datum values ``m`` [Nc, D] with bandwidths ``h`` [D] and uniforms ``u`` [Nc, D]."""
    m = np.asarray(m, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    Nc, D = m.shape
    r = Draws()
    r.u, r.m = u, m
    r.cands = np.full((Nc, D), np.nan)
    r.zs, r.lo, r.hi, r.ptail = (np.full((Nc, D), np.nan) for _ in range(4))
    r.clamped = np.zeros((Nc, D), dtype=bool)
    r.near_edge = np.zeros((Nc, D), dtype=bool)
    r.domain = np.zeros((Nc, D), dtype=bool)
    with np.errstate(all="ignore"):
        for d in range(D):
            t, hd, md, ud = int(levels[d]), h[d], m[:, d], u[:, d]
            rh = np.float64(1.0) / hd
            if t > 0:
                thr = np.float64(1.0) - hd
                keep = ud < thr
                v = (ud - thr) * rh if thr > 0 else ud
                vt = v * np.float64(t)
                lv = np.minimum(np.where(keep, 0.0, vt).astype(np.int64), t - 1)
                r.cands[:, d] = np.where(keep, md, lv.astype(np.float64))
                r.near_edge[:, d] = (np.abs(ud - thr) < EDGE) | (~keep & (np.abs(vt - np.rint(vt)) < EDGE))
                continue
            a, b = -md * rh, (1.0 - md) * rh
            ok = a < b
            flip = a > 0
            lo, hi = np.where(flip, -b, a), np.where(flip, -a, b)
            plo, phi = ndtr(lo), ndtr(hi)
            p = plo + ud * (phi - plo)
            up = p > 0.5
            pt = np.where(up, 1.0 - p, p)
            z = ndtri(pt)
            z = np.where(up, -z, z)
            zc = np.minimum(np.maximum(z, lo), hi)
            zs = np.where(flip, -zc, zc)
            x = md + (bw_factor * hd) * zs
            r.cands[:, d] = np.where(ok, x, np.nan)
            r.domain[:, d] = ~ok
            r.zs[:, d] = np.where(ok, zs, np.nan)
            r.lo[:, d] = np.where(ok, np.where(flip, -hi, lo), np.nan)  # the bounds of zs
            r.hi[:, d] = np.where(ok, np.where(flip, -lo, hi), np.nan)
            r.ptail[:, d] = np.where(ok, pt, np.nan)
            r.clamped[:, d] = ok & (zc != z)
    r.err = r.domain.any(axis=1).astype(np.uint8)
    return r


def sample(X, rows, bw, levels, bw_factor, seed, counter_base, stream_id, Nc):
    """hbx_kde_sample: Nc candidates around the observations X[rows] (X [N, D] float64, rows int64 [n])."""
    X = np.asarray(X, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    ctrs = candidate_counters(counter_base, Nc)
    datum = datum_index(seed, ctrs, stream_id, len(rows))
    r = draw(X[rows[datum]], bw, levels, bw_factor, uniforms(seed, ctrs, stream_id, X.shape[1]))
    r.datum = datum
    return r


def sample_groups(X, seg_off, order, n_good, bw_good, levels, bw_factor, seed, counter_base, stream_id, C):
    """hbx_kde_sample_groups: per group b, C candidates around the rows order[seg_off[b]:][:n_good[b]] of its
    segment, candidate (b, i) on the counter counter_base + b C + i; None for a group without a model
    (n_good[b] <= 0 or larger than the segment: NaN rows, no error byte).  With S requests of pool size C0 call
    it with C = S C0: candidate (b, s, i) is then on counter_base + (b S + s) C0 + i."""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for b in range(len(seg_off) - 1):
        s, e, n = int(seg_off[b]), int(seg_off[b + 1]), int(n_good[b])
        if n <= 0 or n > e - s:
            out.append(None)
            continue
        out.append(sample(X[s:e], np.asarray(order[s:s + n]), bw_good[b], levels, bw_factor, seed,
                          int(counter_base) + b * int(C), stream_id, C))
    return out
