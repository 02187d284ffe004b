#!/usr/bin/env python
"""CPU fp64 probe of the staged acquisition's selection (hbx_staged.hip) on the bench stream: how many
candidates the good KDE alone cannot rule out.

    python tools/staged_survivors.py [--cand 1000000] [--obs 10000] [--dc 24] [--du 8] [--levels 4]

BOHB's score is max(1e-8, g) / max(l, 1e-8), so score_i >= 1e-8 / max(l_i, 1e-8) whatever g is.  The probe
scores l for every candidate of bench.py's stream (synthetic.make_candidates_blocked) with the C oracle in the
reference's fp64 arithmetic, g for the seed band l >= l_max / 4, takes U = the seeds' best score, adds the
candidates whose l-only bound is <= U (g scored for them too, so the winner is known) and prints the counts the
GPU stages work with: seeds, survivors at U, at 1.1 U and at 10 U, the winner and its rank by l, the share of
candidates with l < 1e-8.  No GPU, nothing outside the repository (the C oracle builds itself with the system
compiler).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
    a = ap.parse_args(argv)
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
