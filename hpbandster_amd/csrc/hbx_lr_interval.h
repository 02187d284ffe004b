// hbx_lr_interval.h -- the interval of s = ln g - ln l, with no floor, from two fp32 estimates: the device arithmetic the
// log-ratio routes screen by.  Users: hbx_groups_impl.h (grp_emit_lr, the grouped screens' <.., LR = true> instances)
// and hbx_acquire_lr.hip (kde_combine_lr_kernel, the single-pool acquisition).  One derivation, so both routes list and
// discard by the same numbers.
#pragma once
#include "hbx_common.h"

// fp64 -> fp32 rounded towards -inf / +inf: the cast rounds to nearest, so where it came out on the wrong side of v
// it is moved one step along hbx_f2ord's order (monotonic over all floats, the sign change and the infinities included)
__device__ __forceinline__ float grp_f32_down(double v) {
  const float f = (float)v;
  return (double)f > v ? hbx_ord2f(hbx_f2ord(f) - 1u) : f;
}
__device__ __forceinline__ float grp_f32_up(double v) {
  const float f = (float)v;
  return (double)f < v ? hbx_ord2f(hbx_f2ord(f) + 1u) : f;
}

// The interval of ln P, P = S+ - S- the signed sum of one KDE, from its estimate {lpos = ln S+, lneg = ln S-, e = err}
// (both with the normaliser added, rounded to fp32).  The screens' bound says each true sum lies within a factor
// (1 +- e) of the estimated one, so
//     P in [S+ (1 - e) - S- (1 + e),  S+ (1 + e) - S- (1 - e)].
// The estimate holds no linear-domain value (the running maximum is an integer exponent, the sums were turned into
// logs), so both ends are formed in the log domain, in fp64, around the larger of the two logs, hi:
//     r = exp(lo - hi) <= 1 (the smaller sum over the larger),
//     ln |P|_hi = hi + log1p(+e - r_lo (1 - e)),      ln |P|_lo = hi + log1p(-e - r_hi (1 + e))   (argument > -1),
// and the sign of P is that of the larger sum when the lower end exists, unknown otherwise.  Without negative terms
// (lneg = -inf) r = 0: ln P in [lpos + log1p(-e), lpos + log1p(e)].
// What the fp32 logs lost, put back outward:
//   - lpos and lneg were rounded to fp32 once, each off by at most 2^-24 |value|.  r therefore carries a factor within
//     exp(+-dd), dd = 2^-23 (|lpos| + |lneg|) + 2^-40 (twice the roundings: the fp64 subtraction and exp sit in the
//     other half); r_lo = r (1 - dd) <= r exp(-dd) and r_hi = r (1 + 1.02 dd) >= r exp(dd) for dd <= 0.03 -- a
//     candidate with a larger dd is not certified.
//   - the base hi is off by the same rounding: sl = 2^-23 |hi| + 2^-20 is taken from the lower end and added to the
//     upper one; the 2^-20 (1e-6) covers the fp64 evaluation of log1p and exp, the normaliser's fp64 roundings and the
//     difference between the true pdf and the exact re-score's value (grp_exact_rel, 1e-13), with four decimal orders
//     to spare.
// `neg`: the KDE has a negative match factor.  Its exact value is ln of the linear fp64 pdf as it is, so a bound is
// only worth something while that pdf is a normal number: below ln p = -700 the candidate is not certified.  (Without
// a negative factor the re-score takes the log-space value there, which the bound does cover.)  Above +700 nothing is
// certified either.
// Returns sg: +1 P certainly positive, ln P in [lo, hi]; 0 the interval holds 0, ln max(P, 0) <= hi; -1 P certainly
// negative and far from underflow; 2 not usable.
struct GrpLnIv {
  double lo, hi;
  int sg;
};
__device__ __forceinline__ GrpLnIv grp_ln_interval(const KdeEst e, bool neg) {
  GrpLnIv v;
  v.lo = v.hi = NAN;
  v.sg = 2;
  const double lp = (double)e.lpos, ln = (double)e.lneg, er = (double)e.err;
  if (!(lp == lp) || !(ln == ln) || !(er >= 0.0 && er < 0.9)) return v;
  const double hi = fmax(lp, ln), lo = fmin(lp, ln);
  if (!(hi > -INFINITY && hi < INFINITY)) return v;  // (no term at all, or an overflow)
  const double dd = 0x1p-23 * (fabs(lp) + (ln > -INFINITY ? fabs(ln) : 0.0)) + 0x1p-40;
  if (!(dd <= 0.03)) return v;
  const double r = lo > -INFINITY ? exp(lo - hi) : 0.0;
  const double sl = 0x1p-23 * fabs(hi) + 0x1p-20;
  const double ahi = er - r * (1.0 - dd) * (1.0 - er), alo = -er - r * (1.0 + 1.02 * dd) * (1.0 + er);
  const double mhi = hi + log1p(ahi) + sl;
  const double mlo = alo > -1.0 + 0x1p-40 ? hi + log1p(alo) - sl : -INFINITY;
  if (!(mhi < 700.0)) return v;
  if (mlo == -INFINITY) {  // the sign is open: usable (as "may be 0") only where the positive sum is the larger one
    if (lp < ln) return v;
    v.sg = 0;
    v.lo = -INFINITY;
    v.hi = mhi;
    return v;
  }
  if (lp < ln) {  // certainly negative -- NaN by definition, provided the exact pdf cannot underflow to -0
    if (mlo > -700.0) v.sg = -1;
    return v;
  }
  if (neg && !(mlo > -700.0)) return v;
  v.sg = 1;
  v.lo = mlo;
  v.hi = mhi;
  return v;
}
// The interval of s = ln g - ln l from both KDEs' intervals (l not usable is the caller's case: uncertified / forced).
// slo = ln g_lo - ln l_hi, shi = ln g_hi - ln l_lo in fp64; the subtraction's own rounding (2^-53 relative) is inside
// the ends' 2^-20, and the narrowing to fp32 is made outward, so where both signs are certain [slo, shi] holds the
// re-score's s.  kind:
//   LR_IV_FORCE  l may be 0, or l or g is not usable: nothing is known, the candidate is always re-scored
//   LR_IV_NAN    l or g certainly negative: s is NaN, never picked and not re-scored
//   LR_IV_OK     [slo, shi]; a g whose interval holds 0 may as well be negative (s NaN): [-inf, +inf], always listed,
//                and its upper end never lowers a bound taken over the pool
enum { LR_IV_OK = 0, LR_IV_FORCE = 1, LR_IV_NAN = 2 };
struct LrIv {
  float slo, shi;
  int kind;
};
__device__ __forceinline__ LrIv lr_s_interval(const GrpLnIv l, const GrpLnIv g) {
  LrIv o;
  o.slo = o.shi = NAN;
  o.kind = LR_IV_FORCE;
  if (l.sg == 2 || g.sg == 2 || l.sg == 0) return o;
  o.kind = LR_IV_NAN;
  if (l.sg < 0 || g.sg < 0) return o;
  o.kind = LR_IV_OK;
  o.slo = g.sg == 0 ? -INFINITY : grp_f32_down(g.lo - l.hi);
  o.shi = g.sg == 0 ? INFINITY : grp_f32_up(g.hi - l.lo);  // (g may be negative: s may be NaN, nothing bounds it above)
  return o;
}
