// hbx_acq_impl.h -- device arithmetic shared by the acquisition's selection steps: the argmin's
// (hbx_kde.hip: combine, final) and the top-k's (hbx_topk.hip: bounds, final).  One definition of the
// score interval, the score and its error bound, so both paths screen and rank by the same numbers.
#pragma once
#include "hbx_kde_impl.h"
#include "hbx_score.h"  // OBS_SPLIT_MAX

// ln-pdf interval [lo, hi] and point estimate from (ln S+, ln S-, relative bound); -inf means pdf <= 0
__device__ __forceinline__ void est_interval(const KdeEst e, float* lo, float* hi, float* pt) {
  const float m = fmaxf(e.lpos, e.lneg);
  if (m == -INFINITY) {
    *lo = *hi = *pt = -INFINITY;
    return;
  }
  const float a = __expf(e.lpos - m), b = __expf(e.lneg - m);
  const float S = a - b, E = e.err * (a + b) + 1e-6f * (a + b);
  *pt = S > 0.f ? m + __logf(S) : -INFINITY;
  *hi = (S + E) > 0.f ? m + __logf(S + E) + 1e-6f * fabsf(m) + 1e-5f : -INFINITY;
  *lo = (S - E) > 0.f ? m + __logf(S - E) - 1e-6f * fabsf(m) - 1e-5f : -INFINITY;
}

// Interval [slo, shi] of ln(max(f, g) / max(l, f)) (bohb.py:129; f: the score floor F, 1e-8 in the reference
// snapshot) of one candidate from its two estimates a (l) and b (g), with the ln-pdf point estimates.
//   lnan: l is NaN -> max(l, f) is NaN -> the score is NaN (never selected); slo = shi = NaN
//   of:   a pdf's upper bound is past fp64's exp range: the intervals of this call cannot be trusted
//   one:  both factors are certainly clamped: the score is exactly f / f = 1 for every f, slo = shi = 0
struct ScoreIv {
  float slo, shi, lpt, gpt;
  bool lnan, of, one;
};
__device__ __forceinline__ ScoreIv score_interval(const KdeEst a, const KdeEst b, const ScoreFloor F) {
  const float C = F.C;
  ScoreIv v;
  v.of = false;
  v.one = false;
  v.lnan = a.lpos != a.lpos;
  float llo, lhi, glo, ghi;
  if (v.lnan) {
    v.slo = v.shi = NAN;
    v.lpt = NAN;
    est_interval(b, &glo, &ghi, &v.gpt);
    if (b.lpos != b.lpos) v.gpt = NAN;
    return v;
  }
  est_interval(a, &llo, &lhi, &v.lpt);
  float Glo, Ghi;
  if (b.lpos != b.lpos) {  // g NaN -> max(f, g) == f
    Glo = Ghi = C;
    v.gpt = NAN;
  } else {
    est_interval(b, &glo, &ghi, &v.gpt);
    Glo = fmaxf(glo, C);
    Ghi = fmaxf(ghi, C);
    v.of = ghi > 700.f;
  }
  v.of = v.of || lhi > 700.f;
  v.slo = Glo - fmaxf(lhi, C) - F.w;
  v.shi = Ghi - fmaxf(llo, C) + F.w;
  const float C1 = F.C1;  // C less the margin for the rounding of ln f to float (ScoreFloor)
  if (lhi < C1 && (b.lpos != b.lpos || ghi < C1)) {  // both clamped: score exactly 1 (ln 0)
    v.one = true;
    v.slo = v.shi = 0.f;
  }
  return v;
}

// The staged acquisition (hbx_staged.hip) did not evaluate g for this candidate: err of its a.eg entry (distinct
// from the rescue marker -1 and exact-only's -2).  Its score interval from l alone: whatever g is,
// max(f, g) >= f, so slo = C - max(lhi, C) (less F.w); no upper end (shi = +inf never lowers U), never a certain
// tie.  lnan and of come from l as in score_interval.
#define HBX_EST_NOT_EVAL (-3.f)
__device__ __forceinline__ ScoreIv score_interval_l_only(const KdeEst a, const ScoreFloor F) {
  const float C = F.C;
  ScoreIv v;
  v.of = false;
  v.one = false;
  v.gpt = NAN;
  v.lnan = a.lpos != a.lpos;
  if (v.lnan) {
    v.slo = v.shi = NAN;
    v.lpt = NAN;
    return v;
  }
  float llo, lhi;
  est_interval(a, &llo, &lhi, &v.lpt);
  v.of = lhi > 700.f;
  v.slo = C - fmaxf(lhi, C) - F.w;
  v.shi = INFINITY;
  return v;
}

// Candidate i's estimate merged over its nsplit observation-split partials (hbx_score_h32.hip; partial r at
// e[r stride + i]): the sums add (log domain, fp32); each partial's relative bound holds for the total too (sums
// of positive terms), plus per merge its own rounding: 2^-18 for the fp32 exp / log / addition, and the rounding
// of the merged ln S to fp32 (<= |ln S| 2^-23 absolute, counted as 2^-22 |ln S| relative on S)
__device__ __forceinline__ KdeEst merge_loaded_splits(const KdeEst (&p)[OBS_SPLIT_MAX], int nsplit) {
  auto lae = [](float x, float y) {
    const float m = fmaxf(x, y);
    return m == -INFINITY ? m : m + __logf(__expf(x - m) + __expf(y - m));
  };
  KdeEst a = p[0];
#pragma unroll
  for (int r = 1; r < OBS_SPLIT_MAX; ++r) {
    if (r < nsplit) {
      const KdeEst b = p[r];
      if (a.lpos != a.lpos || b.lpos != b.lpos) {  // structural NaN (every split carries it)
        a.lpos = NAN;
      } else {
        a.lpos = lae(a.lpos, b.lpos);
        a.lneg = lae(a.lneg, b.lneg);
        const float ml = fmaxf(a.lpos > -INFINITY ? fabsf(a.lpos) : 0.f, a.lneg > -INFINITY ? fabsf(a.lneg) : 0.f);
        a.err = fmaxf(a.err, b.err) + 0x1p-18f + ml * 0x1p-22f;
      }
    }
  }
  return a;
}
// every partial's load issued before the first merge (a load per dependent merge step cost 14 us for 16
// splits of 64 candidates); fixed-size and fully unrolled, so the partials stay in registers
__device__ __forceinline__ void load_splits(KdeEst (&p)[OBS_SPLIT_MAX], const KdeEst* __restrict__ e, int64_t stride,
                                            int64_t i, int nsplit) {
#pragma unroll
  for (int r = 0; r < OBS_SPLIT_MAX; ++r) p[r] = r < nsplit ? e[(int64_t)r * stride + i] : kde_est_neutral();
}
__device__ __forceinline__ KdeEst merge_splits(const KdeEst* __restrict__ e, int64_t stride, int64_t i, int nsplit) {
  KdeEst p[OBS_SPLIT_MAX];
  load_splits(p, e, stride, i, nsplit);
  return merge_loaded_splits(p, nsplit);
}
// The same for a list launch's partials, where a rescue marker (err == -1) in any partial makes the merged
// estimate the marker: the marker test on the partials already loaded, not on a second, one-by-one read of them.
__device__ __forceinline__ KdeEst merge_splits_or_marker(const KdeEst* __restrict__ e, int64_t stride, int64_t i,
                                                         int nsplit, bool* mark) {
  KdeEst p[OBS_SPLIT_MAX];
  load_splits(p, e, stride, i, nsplit);
  bool m = false;
#pragma unroll
  for (int r = 0; r < OBS_SPLIT_MAX; ++r) m = m || (r < nsplit && p[r].err == -1.f);
  *mark = m;
  const KdeEst a = merge_loaded_splits(p, nsplit);
  return m ? KdeEst{0.f, -INFINITY, -1.f, 0.f} : a;
}

// bohb.py:129 with Python max() and the score floor f: max(f, g) keeps f unless g > f (NaN -> f); max(l, f)
// keeps l unless f > l (NaN -> NaN).  Scores are >= 0 or NaN (the numerator is >= f > 0; an l of +inf gives +0,
// g = l = inf gives NaN), so the bits of a non-NaN score order like the score.
__device__ __forceinline__ double bohb_score(double g, double l, double f) {
  return ((g > f) ? g : f) / ((f > l) ? f : l);
}

// Bound of |exact pdf here - pdf in numpy's arithmetic| / pdf for one KDE at one candidate.  Both run
// the same IEEE operations in the same order (SM:_kernel_base.py:509-516: per-dim kernels, dim-ordered
// product, / prod(bw_c), numpy's pairwise sum, / n) except exp, where ocml's and numpy's results may
// differ by ulps: per term <= (6 D + 4) u, plus 2 u per level of the summation tree (<= 40 levels up
// to 1e5 observations) -- (8 D + 160) 2^-52 leaves a margin over both.  Sums with negative terms
// (categorical bandwidth > 1) scale by their condition number sum|t| / |sum t|, taken pessimistically
// from the fp32 estimate (inf when its sign is not certain).
__device__ __forceinline__ double exact_rel(const KdeParams* __restrict__ P, const KdeEst e) {
  const double base = (8.0 * (double)P->D + 160.0) * 0x1p-52;
  if (!P->has_neg) return base;
  if (e.err < -1.5f) return INFINITY;  // exact-only acquisition: no fp32 estimate of the condition
  const float m = fmaxf(e.lpos, e.lneg);
  if (!(m > -INFINITY)) return base;
  const float a = __expf(e.lpos - m), b = __expf(e.lneg - m);
  const float den = fabsf(a - b) - (e.err + 1e-6f) * (a + b);
  if (!(den > 0.f)) return INFINITY;
  return base * (double)((a + b) / den) * 1.01;
}

// relative bound of one candidate's score (bohb.py:129: g clamped, / l clamped): both pdfs' bounds
// plus the division's rounding
__device__ __forceinline__ double score_rel(const KdeParams* __restrict__ Pg, const KdeParams* __restrict__ Pb,
                                            const KdeEst* __restrict__ el, const KdeEst* __restrict__ eg,
                                            int64_t i) {
  return exact_rel(Pg, el[i]) + exact_rel(Pb, eg[i]) + 0x1p-51;
}

// p may beat the winner in numpy's arithmetic only if s_p (1 - R_p) <= s_best (1 + R_best)
__device__ __forceinline__ bool near_best(double s, double rp, double best, double rb) {
  return s < INFINITY && s <= best * (1.0 + 1.0001 * (rp + rb));
}
