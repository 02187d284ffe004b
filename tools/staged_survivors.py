#!/usr/bin/env python
"""CPU fp64 probe of the staged acquisition's selection (hbx_staged.hip) on the bench stream: how many
candidates the good KDE alone cannot rule out.

    python tools/staged_survivors.py [--cand 1000000] [--obs 10000] [--dc 24] [--du 8] [--levels 4] [--topk K[,K...]]

BOHB's score is max(1e-8, g) / max(l, 1e-8), so score_i >= 1e-8 / max(l_i, 1e-8) whatever g is.  The probe
scores l for every candidate of bench.py's stream (synthetic.make_candidates_blocked) with the C oracle in the
reference's fp64 arithmetic, g for the seed band l >= l_max / 4, takes U = the seeds' best score, adds the
candidates whose l-only bound is <= U (g scored for them too, so the winner is known) and prints the counts the
GPU stages work with: seeds, survivors at U, at 1.1 U and at 10 U, the winner and its rank by l, the share of
candidates with l < 1e-8.  No GPU, nothing outside the repository (the C oracle builds itself with the system
compiler).

--topk: the staged top-k's selection (hbx_topk.hip "Staged scoring") instead, one line per k as it goes: the seed
band l >= L_(k+1) / 4 around the (k+1)-th largest l (at most the seed list's 4096 candidates), U_(k+1) = the
(k+1)-th smallest score among the seeds, and the unseeded candidates whose l-only bound is <= U_(k+1).  The rule
itself is the numpy functions below (tests/test_staged_topk_host.py checks them against brute force).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


LIST_CAP = 4096  # STAGED_LIST_CAP (hbx_acquire.h): seeds at most
MAX_K = 1024     # HBX_TOPK_MAX_K (include/hbx.h)


def bohb_scores(l, g):
    """max(1e-8, g) / max(l, 1e-8) with Python's max (bohb.py:129): NaN g -> 1e-8, NaN l -> NaN."""
    l, g = np.asarray(l, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(g > 1e-8, g, 1e-8) / np.where(1e-8 > l, 1e-8, l)


def _check_k(k):
    if int(k) != k or k < 1 or k > MAX_K:
        raise ValueError("k must be an integer in [1, %d], got %r" % (MAX_K, k))
    return int(k)


def topk_seed_band(l, k):
    """(L, band): L = the (k+1)-th largest l over the candidates whose l is not NaN and band = the indices with
    l >= L / 4, ascending; with fewer than k+1 such candidates L is None and the band is all of them."""
    k = _check_k(k)
    l = np.asarray(l, dtype=np.float64)
    if l.ndim != 1:
        raise ValueError("l must be one-dimensional")
    ok = np.nonzero(~np.isnan(l))[0]
    if len(ok) < k + 1:
        return None, ok
    L = np.partition(l[ok], len(ok) - (k + 1))[len(ok) - (k + 1)]
    return float(L), ok[l[ok] >= L / 4]


def topk_u(seed_scores, k):
    """U_(k+1): the (k+1)-th smallest of the seeds' scores that are not NaN, +inf with fewer than k+1."""
    k = _check_k(k)
    s = np.asarray(seed_scores, dtype=np.float64)
    s = s[~np.isnan(s)]
    return float(np.partition(s, k)[k]) if len(s) >= k + 1 else float("inf")


def topk_select(l, g_of, k, seeds=None):
    """The staged top-k's selection over l (every candidate) and g_of(indices) -> g (called for the evaluated
    candidates only): dict(L, seeds, U, survivors, evaluated, top) with top = the first k evaluated indices by
    (score, index), NaN scores left out.  seeds: any subset of the band (default: its first LIST_CAP indices) --
    at least k+1 of them, or the whole band where it is smaller."""
    k = _check_k(k)
    l = np.asarray(l, dtype=np.float64)
    L, band = topk_seed_band(l, k)
    if seeds is None:
        seeds = band[:LIST_CAP]
    seeds = np.unique(np.asarray(seeds, dtype=np.int64))
    if len(np.setdiff1d(seeds, band)) or len(seeds) > LIST_CAP:
        raise ValueError("the seeds must be at most %d candidates of the band" % LIST_CAP)
    if len(seeds) < min(k + 1, len(band)):
        raise ValueError("fewer than k + 1 seeds from a band that holds them")
    g_seed = np.asarray(g_of(seeds), dtype=np.float64)
    U = topk_u(bohb_scores(l[seeds], g_seed), k)
    with np.errstate(invalid="ignore"):
        keep = 1e-8 / np.where(1e-8 > l, 1e-8, l) <= U  # NaN l: never; '<=': ties survive
    keep[seeds] = False
    surv = np.nonzero(keep)[0]
    ev = np.concatenate([seeds, surv])
    s = np.concatenate([bohb_scores(l[seeds], g_seed), bohb_scores(l[surv], g_of(surv))])
    ok = ~np.isnan(s)
    ev_ok, s_ok = ev[ok], s[ok]
    order = np.lexsort((ev_ok, s_ok))[:k]
    return {"L": L, "seeds": seeds, "U": U, "survivors": surv, "evaluated": ev, "top": ev_ok[order],
            "scores": s_ok[order]}


def brute_topk(l, g, k):
    """The first k indices by (score, index) over every candidate with a score: what topk_select must return."""
    s = bohb_scores(l, g)
    ok = np.nonzero(~np.isnan(s))[0]
    return ok[np.lexsort((ok, s[ok]))[:_check_k(k)]]


def main(argv=None):
    from hpbandster_amd import synthetic as S
    from oracle import c_oracle
    from oracle import kde_oracle as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cand", type=int, default=1000000)
    ap.add_argument("--obs", type=int, default=10000)
    ap.add_argument("--dc", type=int, default=24)
    ap.add_argument("--du", type=int, default=8)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--block", type=int, default=1 << 16, help="candidates scored per oracle call")
    ap.add_argument("--topk", default=None, help="k or k,k,...: the staged top-k's selection instead of the argmin's")
    a = ap.parse_args(argv)
    ks = [_check_k(int(k)) for k in a.topk.split(",")] if a.topk else []
    D = a.dc + a.du
    vt = S.var_type_string(a.dc, a.du)
    X = S.make_observations(a.obs, a.dc, a.du, a.levels)
    g_idx, b_idx = O.bohb_split(X, S.make_losses(a.obs), D + 1)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)
    t0 = time.time()
    l = np.empty(a.cand)
    for lo in range(0, a.cand, a.block):
        hi = min(a.cand, lo + a.block)
        C = S.make_candidates_blocked(lo, hi, a.dc, a.du, a.levels)
        l[lo:hi] = c_oracle.kde_pdf(X[g_idx], bwg, vt, nlg, C, exact=True)
    print("l of %d candidates against %d good observations: %.0f s" % (a.cand, len(g_idx), time.time() - t0))

    if ks:
        known = {}  # candidate -> g, shared by the ks

        def g_block(idx):
            """g of candidates idx, one oracle call per block of the stream that holds new ones."""
            idx = np.asarray(idx, dtype=np.int64)
            new = np.array(sorted(set(idx.tolist()) - set(known)), dtype=np.int64)
            for b in np.unique(new // S.CAND_BLOCK):
                rows = new[new // S.CAND_BLOCK == b]
                blk = S.make_candidates_blocked(int(b) * S.CAND_BLOCK, min(a.cand, (int(b) + 1) * S.CAND_BLOCK), a.dc,
                                                a.du, a.levels)
                gv = c_oracle.kde_pdf(X[b_idx], bwb, vt, nlb, blk[rows - int(b) * S.CAND_BLOCK], exact=True)
                known.update(zip(rows.tolist(), gv.tolist()))
            return np.array([known[i] for i in idx.tolist()], dtype=np.float64)
        print("candidates with l < 1e-8: %.1f %%" % (100.0 * float((l < 1e-8).mean())), flush=True)
        for k in ks:
            t1 = time.time()
            r = topk_select(l, g_block, k)
            band = len(topk_seed_band(l, k)[1])
            print("k %d: L_(k+1) %.4e; band l >= L / 4: %d%s; seeds %d; U_(k+1) %.6g; survivors %d; g needed for %d "
                  "= %.4f %% of the candidates; k-th score %.6g (%.0f s)" %
                  (k, r["L"] if r["L"] is not None else float("nan"), band,
                   " (capped at the list capacity)" if band > LIST_CAP else "", len(r["seeds"]), r["U"],
                   len(r["survivors"]), len(r["evaluated"]), 100.0 * len(r["evaluated"]) / a.cand,
                   r["scores"][-1] if len(r["scores"]) else float("nan"), time.time() - t1), flush=True)
        return 0

    def g_of(idx):
        out = np.empty(len(idx))
        for k, i in enumerate(idx):
            C = S.make_candidates_blocked(int(i), int(i) + 1, a.dc, a.du, a.levels)
            out[k] = c_oracle.kde_pdf(X[b_idx], bwb, vt, nlb, C, exact=True)[0]
        return out

    def score(lv, gv):
        return np.maximum(gv, 1e-8) / np.maximum(lv, 1e-8)
    lmax = np.nanmax(l)
    seeds = np.nonzero(l >= lmax / 4)[0]
    s_seed = score(l[seeds], g_of(seeds))
    U = s_seed.min()
    bound = 1e-8 / np.maximum(l, 1e-8)  # NaN l: NaN, never <=
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(bound <= U)[0]
    extra = np.setdiff1d(cand, seeds)
    s_all = np.concatenate([s_seed, score(l[extra], g_of(extra))])
    idx_all = np.concatenate([seeds, extra])
    order = np.lexsort((idx_all, s_all))
    win, best = int(idx_all[order[0]]), float(s_all[order[0]])
    with np.errstate(invalid="ignore"):
        print("l_max %.4e; seeds (l >= l_max / 4): %d; U_seed %.6g" % (lmax, len(seeds), U))
        print("winner %d: score %.6g, l %.4e, rank by l %d" % (win, best, l[win], int((l > l[win]).sum()) + 1))
        for f in (1.0, 1.1, 10.0):
            print("candidates with 1e-8 / max(l, 1e-8) <= %.1f x best score: %d of %d" %
                  (f, int((bound <= f * best).sum()), a.cand))
        print("survivors beside the seeds at U_seed: %d; g needed for %d candidates = %.4f %% of the pairs' bad part"
              % (len(extra), len(idx_all), 100.0 * len(idx_all) / a.cand))
        print("candidates with l < 1e-8 (l-only bound: a score >= 1): %.1f %%" % (100.0 * float((l < 1e-8).mean())))


if __name__ == "__main__":
    sys.exit(main())
