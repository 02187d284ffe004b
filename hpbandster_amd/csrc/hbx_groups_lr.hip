// hbx_groups_lr.hip -- grouped acquisition by log ratio: per request the first index minimising s = ln g - ln l, with
// no floor (hbx_kde_acquire_groups_batch_lr; bohb.py:124-169 with the score read in the log domain).
//
// The floored score max(f, g) / max(l, f) is exactly 1 wherever both densities lie under f -- nearly everywhere at
// config #5's 32 dims -- and its strict argmin then returns candidate 0.  s still orders those candidates.  The call is
// an acquisition like the floored one: screen, shortlist, exact re-score, strict argmin; it does not form ln-pdfs of
// every candidate.
//
//   screen   the screens of hbx_groups.hip, their <.., LR = true> instances: the same loop, staging and bound, then
//            grp_emit_lr (hbx_groups_impl.h; the derivation stands there): [slo, shi] around ln g - ln l, GS_FORCE
//            where l may be 0 or nothing is certified, GS_NAN where l or g is certainly negative, [-inf, +inf] where g
//            may be negative (listed, but its upper end says nothing: s may be NaN).
//   select   groups_select_lr_kernel<MASK> below, one block of GRP_SEL_THREADS per request q = b S + s, laid out as
//            groups_select_kernel is (status, skipped and empty records, counters).
//            pass 1   U = min shi over the certified candidates (no GS_FORCE, no GS_NAN).
//            pass 2   the shortlist {slo <= U} plus the forced candidates, in index order (grp_compact); exact-only
//                     groups list everything.  Every entry gets both exact fp64 pdfs (grp_exact_both, the reference's
//                     values bit for bit), then per KDE k
//                         L_k = log(p_k)            p_k a positive normal number (or +inf)
//                         L_k = NaN                 p_k negative or NaN
//                         L_k = grp_logspace_ln     p_k zero or subnormal, KDE without a negative match factor
//                         L_k = log(p_k)            p_k zero or subnormal, KDE with one (-inf for 0)
//                     and s = L_g - L_l.  The log-space value is below ln of the smallest normal (its pdf underflowed),
//                     so the two forms order consistently.
//            order    hbx_kde_rank_groups' for k = 1: the key hbx_d2ord(s) -- finite and -inf by value, -0 as +0, +inf
//                     behind them, NaN never picked -- and the lower index among equal keys (thread 0 walks the
//                     shortlist in index order with a strict '<').  All NaN: index -1, the finish step's NO_SCORE rule.
//            record   index, score = s, the exact pdf_l / pdf_g, shortlist, rel; near = the re-scored candidates with
//                     s <= s_best + 1.0001 (rel + rel_best), HBX_ACQ_NEAR_TIE when more than one; HBX_ACQ_OVERFLOW for
//                     exact-only groups; HBX_ACQ_LOG_RATIO on every record this kernel answers (not on skipped ones).
//                     The exact s stay in the candidates' GScreen slots for the near count, as in the floored select.
//   counters the workspace head's words [0 .. 3] as hbx_kde_acquire_groups_batch_m counts them (the public ones), and
//            two internal ones for tools/bench_groups.py: [4] log-space evaluations, [5] forced candidates re-scored.
//
// grp_logspace_ln -- ln of an underflowed pdf.  Converged runs have tiny bandwidths; a far candidate's exact g is then
// 0, s = -inf, and several such candidates would tie on the first index: the floored score's defect one level down.
// The block's threads split the KDE's n rows (thread i: rows i, i + T, ...).  Per pair, in fp64, by direct differences,
//     t = sum_c -(x_c - X_jc)^2 / (2 h_c^2) + sum_u ([match] ln(1 - h_u) + [no match] ln(h_u / (c_u - 1)))
// (the per-dim constants are exact_setup's, the categorical ones turned into logs once per evaluation).  Each thread
// keeps a running sum of exp2(t log2 e - m) against an INTEGER running maximum m = max ceil(t log2 e), so every rescale
// is an exact ldexp; thread 0 merges the T partials from LDS in thread order, again by ldexp -- no atomics, so two runs
// give the same bytes -- and adds ln of the normaliser, -ln n - sum_c ln h_c - dc ln sqrt(2 pi).  A pair whose t is NaN
// or +inf (a mismatch in a single-level dim: 0 / 0) makes the value NaN, as the reference's pdf is.
// Error bound (u = 2^-53), absolute, on the returned ln p:
//     - t: per continuous dim a subtraction, a square, a division and an addition, per categorical dim an addition of a
//       log rounded once; every partial sum is at most max|t| in magnitude, and the change to log2 units and the
//       subtraction of m add two roundings of that size: (dc + du + 2) u max|t| on the exponent, in ln units.
//     - the sum: each term exp2() within 1 ulp (2 u relative), each of the n additions u, the merge of T partials T u
//       more, log2 of the sum and the two final additions a few u of |ln p| <= max|t|: (n + T) 2^-52 covers them.
//     => |ln p here - ln p| <= (dc + du + 2) 2^-53 max|t| + (n + T) 2^-52.
//   At n = 1e3, D = 32, T = 256 and max|t| = 1e4 (an underflowed pdf starts at |t| = 708) that is 3.8e-11 + 2.8e-13.
//   The bound is added to the candidate's rel, so the near count sees it.
#include <float.h>

#include "hbx_groups_acq.h"

#define LR_T GRP_SEL_THREADS

// ln of KDE v's pdf at x in fp64 log space (header); whole block, the value and its bound are valid in thread 0.
// s_m, s_s: LR_T doubles of LDS each; s_tmax: the pairs' max |t| (non-negative doubles order as their bits).
__device__ double grp_logspace_ln(const GrpView* v, int D, const double* __restrict__ x, const double* __restrict__ Xs,
                                  const int64_t* __restrict__ rows, ExactShared* sh, double* s_m, double* s_s,
                                  unsigned long long* s_tmax, double* bound) {
  const int tid = threadIdx.x;
  exact_setup(v, D, x, sh);  // c0 = 2 h^2 | 1 - h, c1 = h / (c - 1), xd = x; ends with a barrier
  for (int d = tid; d < D; d += LR_T)
    if (!sh->cont[d]) {
      sh->c0[d] = log(sh->c0[d]);  // (1 - h >= 0 here; ln 0 = -inf: a match contributes nothing)
      sh->c1[d] = log(sh->c1[d]);
    }
  if (tid == 0) *s_tmax = 0ull;
  __syncthreads();
  const int n = v->n;
  double m = -INFINITY, s = 0.0, tmax = 0.0;
  bool bad = false;
  for (int j = tid; j < n; j += LR_T) {
    const double* xr = Xs + rows[j] * (int64_t)D;
    double t = 0.0;
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      const double xv = sh->xd[d], o = xr[d];
      if (sh->cont[d]) {
        const double diff = o - xv;
        t -= (diff * diff) / sh->c0[d];
      } else {
        t += (o == xv) ? sh->c0[d] : sh->c1[d];
      }
    }
    if (t != t || t == INFINITY) {
      bad = true;
    } else if (t > -INFINITY) {
      tmax = fmax(tmax, fabs(t));
      const double t2 = t * M_LOG2E, tc = ceil(t2);
      if (tc > m) {  // a new running maximum (integer): exact rescale
        s = ldexp(s, (int)fmax(m - tc, -2000.0));
        m = tc;
      }
      s += exp2(t2 - m);
    }
  }
  s_m[tid] = m;
  s_s[tid] = bad ? NAN : s;
  atomicMax(s_tmax, (unsigned long long)__double_as_longlong(tmax));
  __syncthreads();
  double r = NAN;
  if (tid == 0) {
    double M = -INFINITY, S = 0.0;
    for (int i = 0; i < LR_T; ++i) M = fmax(M, s_m[i]);
    for (int i = 0; i < LR_T; ++i) {
      const double si = s_s[i];
      if (si != si)
        S = NAN;
      else if (s_m[i] > -INFINITY)
        S += ldexp(si, (int)fmax(s_m[i] - M, -2000.0));
    }
    int dc = 0;
    double slh = 0.0;
    for (int d = 0; d < D; ++d)
      if (sh->cont[d]) {
        slh += log(v->bw[d]);
        ++dc;
      }
    const double nrm = -log((double)n) - slh - (double)dc * (0.5 * log(2.0 * M_PI));
    r = (S != S) ? NAN : (S > 0.0 ? (log2(S) + M) * M_LN2 + nrm : -INFINITY);
    *bound = (double)(D + 2) * 0x1p-53 * __longlong_as_double((long long)*s_tmax) + (double)(n + LR_T) * 0x1p-52;
  }
  __syncthreads();  // (sh, s_m, s_s are free again)
  return r;
}

// L of one exact pdf where no log-space value is due: NaN for a negative or NaN pdf, ln p otherwise (-0 -> -inf)
__device__ __forceinline__ double lr_log(double p) { return (p != p || p < 0.0) ? NAN : log(p); }
// zero or a positive subnormal: the pdf underflowed
__device__ __forceinline__ bool lr_underflowed(double p) { return p >= 0.0 && p < DBL_MIN; }

template <bool MASK>
__global__ __launch_bounds__(LR_T) void groups_select_lr_kernel(GrpArgs A) {
  __shared__ ExactShared sh;
  __shared__ GrpView vw[2];
  __shared__ int32_t slist[LR_T];
  __shared__ int32_t swc[LR_T / 64];
  __shared__ double s_m[LR_T], s_s[LR_T];
  __shared__ unsigned long long s_tmax;
  __shared__ uint32_t s_U;
  __shared__ int32_t s_st, s_need, s_nforce;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x, b = q / A.S;  // request q = b S + s of group b
  const int D = A.M.D;
  const int64_t C = A.C;
  if (tid == 0) {
    s_U = hbx_f2ord(INFINITY);
    s_need = 0;
    s_nforce = 0;
  }
  int st;
  if (grp_select_prologue(A, q, b, MASK ? A.want : nullptr, true, HBX_ACQ_LOG_RATIO, &s_st, &st)) return;
  const double* Xs;
  const int64_t *rows_g, *rows_b;
  grp_rows(A.M, b, vw, &Xs, &rows_g, &rows_b);
  GScreen* scr = A.scr + q * C;
  const double* cand = A.cand + q * C * D;
  const bool all = (st & GRP_EXACT_ONLY) != 0;
  // pass 1: U = min shi over the certified candidates
  {
    uint32_t u = hbx_f2ord(INFINITY);
    for (int64_t i = tid; i < C; i += LR_T) {
      const GScreen g = scr[i];
      if (g.fl & (GS_FORCE | GS_NAN)) continue;
      u = min(u, hbx_f2ord(g.shi));
    }
    atomicMin(&s_U, u);
  }
  __syncthreads();  // (also: vw is written)
  const float U = hbx_ord2f(s_U);
  // pass 2: the shortlist in index order, LR_T candidates at a time; each entry's exact pdfs by the whole block
  uint64_t bkey = ~0ull;  // hbx_d2ord of the best s so far (thread 0); every NaN has this key and never wins
  double best = NAN, bl = NAN, bg = NAN;
  int64_t bidx = -1;
  int32_t nshort = 0, nforce = 0, nls = 0;
  for (int64_t c0 = 0; c0 < C; c0 += LR_T) {
    const int64_t i = c0 + tid;
    bool in = false;
    if (i < C) {
      const GScreen g = scr[i];
      in = all || (g.fl & GS_FORCE) || (!(g.fl & GS_NAN) && g.slo <= U);
      nforce += (in && (g.fl & GS_FORCE)) ? 1 : 0;
    }
    const int tot = grp_compact(in, swc, slist);
    for (int p = 0; p < tot; ++p) {
      const int64_t ip = c0 + slist[p];
      const double* x = cand + ip * D;
      double l, g;
      grp_exact_both(vw, D, x, Xs, rows_g, rows_b, &sh, &l, &g);
      if (tid == 0)  // which of the two underflowed in a KDE whose log-space value is defined
        s_need = ((lr_underflowed(l) && !(st & GRP_NEG(0))) ? 1 : 0) | ((lr_underflowed(g) && !(st & GRP_NEG(1))) ? 2 : 0);
      __syncthreads();  // (also: the exact pass has left sh)
      const int need = s_need;
      double Ll = NAN, Lg = NAN, el = 0.0, eg = 0.0;
      if (need & 1) Ll = grp_logspace_ln(&vw[0], D, x, Xs, rows_g, &sh, s_m, s_s, &s_tmax, &el);  // (uniform)
      if (need & 2) Lg = grp_logspace_ln(&vw[1], D, x, Xs, rows_b, &sh, s_m, s_s, &s_tmax, &eg);
      if (tid == 0) {
        if (!(need & 1)) Ll = lr_log(l);
        if (!(need & 2)) Lg = lr_log(g);
        const double s = Lg - Ll;
        if (need) scr[ip].rel = (float)(((double)scr[ip].rel + el + eg) * 1.000001);
        scr[ip].score = s;
        scr[ip].fl |= GS_DONE;
        const uint64_t key = hbx_d2ord(s);
        if (key < bkey) {  // index order: strict '<' keeps the first index
          bkey = key;
          best = s;
          bidx = ip;
          bl = l;
          bg = g;
        }
        nls += (need & 1) + ((need >> 1) & 1);
      }
      __syncthreads();
    }
    nshort += tot;
  }
  if (nforce) atomicAdd(&s_nforce, nforce);
  // near: s <= s_best + 1.0001 (rel + rel_best); w = +inf: no bound, near whatever s is
  auto near = [](double s, double rel, double sb, double rb) {
    const double w = 1.0001 * (rel + rb);
    return s < INFINITY && (w == INFINITY || s <= sb + w);
  };
  grp_select_tail(A, q, scr, C, best, bidx, bl, bg, nshort, HBX_ACQ_LOG_RATIO | (all ? HBX_ACQ_OVERFLOW : 0), 0, near);
  if (tid == 0) {
    atomicAdd(A.stats + 0, 1ull);
    atomicAdd(A.stats + 3, (unsigned long long)nshort);
    if (nls) atomicAdd(A.stats + 4, (unsigned long long)nls);
    if (s_nforce) atomicAdd(A.stats + 5, (unsigned long long)s_nforce);
  }
}

void grp_launch_select_lr(const GrpArgs& A, bool masked, hipStream_t s) {
  hipLaunchKernelGGL((masked ? groups_select_lr_kernel<true> : groups_select_lr_kernel<false>),
                     dim3((unsigned)(A.M.B * A.S)), dim3(LR_T), 0, s, A);
}
