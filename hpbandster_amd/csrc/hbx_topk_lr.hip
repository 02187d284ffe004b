// hbx_topk_lr.hip -- top-k acquisition by log ratio on MI355X (gfx950): the k best candidates of ONE pool by
// s = ln g - ln l, with no floor (hbx_kde_acquire_topk_lr).  What hbx_kde_acquire_topk is to hbx_kde_acquire, for
// hbx_kde_acquire_lr: where both densities lie under the floor the floored score is exactly 1 and the floored top-k
// returns the lowest indices; s still orders those candidates.  Returns the first min(k, F) entries of the ascending
// order by (hbx_d2ord(s), index) over the F candidates whose s is not NaN -- finite values and -inf by value, +inf behind
// them -- in hbx_kde_acquire_topk's result block, score = s, the flags with HBX_ACQ_LOG_RATIO.  Entry 0 is
// hbx_kde_acquire_lr's pick.  All on the caller's stream:
//
//   scoring     acq_plan / acq_score as acquire_lr_impl calls them (hbx_acquire_lr.hip): unstaged -- staging prunes by
//               the floor --, the instance by HBX_LR_COARSE, the rescue pass a launch of its own
//   bounds      topk_bounds_lr_kernel: per candidate the interval of s (hbx_lr_interval.h), lo as the shortlist
//               predicate reads it and the ordered key of shi for the select; kde_combine_lr_kernel's table:
//                   forced (l not usable or may be 0, g not usable)   lo = -inf, key +inf: always listed, never
//                                                                     lowers U_k
//                   l or g certainly negative                         lo = NaN, key +inf: never listed
//                   g may be 0                                        lo = -inf, key +inf
//                   otherwise                                         lo = slo, key of shi
//               It also zeroes the select's histograms.  No overflow flag: per-candidate
//               forcing takes its place.  Exact-only pairs: acq_exact_only_init, the histograms zeroed, everything
//               listed (U_k = +inf), as in the floored top-k.
//   select      topk_hist_kernel x4 and topk_shortlist_kernel (hbx_topk.hip) unchanged: U_k the k-th smallest finite
//               shi, the list {lo not NaN and lo <= U_k}
//   re-score    acq_exact, its unit sums combined: the reference's fp64 pdfs bit for bit
//   ln          acq_lr_ln (kde_lr_ln_kernel, hbx_acquire_lr.hip) over the shortlist: L per entry and KDE, a log-space
//               value where the exact pdf underflowed -- the single call's kernel and bytes.  (A tile of several
//               entries per sweep of a KDE's rows did not fit: two entries need scratch at the two waves per SIMD the
//               LDS allows, four no longer fit the LDS twice per CU; profiles/topk_lr/README.md has the listing.)
//   final       topk_final_lr_kernel: one block, the running best-(k+1) (hbx_topk_rank.h) over the keys
//               hbx_d2ord(L_g - L_l), NaN dropped; the ranked records with score = s, the exact pdfs and
//               rel = score_rel + bnd_l + bnd_g, the absolute bound of s kde_final_lr_kernel reports; HBX_ACQ_NEAR_TIE
//               when an entry and its successor (the last returned one's: the best excluded entry) satisfy
//               s_next <= s + 1.0001 (rel + rel_next), a successor with an infinite bound counting as near.
//
// Why the shortlist holds the whole top-k.  Every certified candidate's s lies in its [lo, shi] (the bounds are
// rigorous: they are what makes the argmin exact).  At least k candidates have shi <= U_k, so at least k values of s
// are <= U_k, so the k-th smallest s is <= U_k.  Every member of the true top-k -- ties by index included, because a
// tied candidate has the same s -- therefore has s <= U_k, hence lo <= U_k, and is re-scored.  A forced candidate, of
// which nothing is known, has lo = -inf and is always re-scored; its key is +inf, so it is not among the k that U_k
// counts, and the argument does not lean on it.  A candidate with lo = NaN has s = NaN and is never returned.  The
// final ranking is over exact values only, so candidates the shortlist holds beyond the top-k cost time, never
// correctness.  With fewer than k finite upper bounds, or an exact-only pair, every candidate whose lo is not NaN is
// re-scored.
//
// Workspace: hbx_kde_lr_workspace_bytes' layout (ws_layout with the lr flag), the keys in the near list's place, then
// the histograms.
#include <float.h>

#include "hbx_acq_impl.h"
#include "hbx_acquire.h"
#include "hbx_host.h"
#include "hbx_lr_interval.h"
#include "hbx_topk_rank.h"

__global__ __launch_bounds__(256) void topk_bounds_lr_kernel(const KdeEst* __restrict__ el,
                                                             const KdeEst* __restrict__ eg, int64_t Nc, int negl,
                                                             int negg, float* __restrict__ lo,
                                                             uint32_t* __restrict__ hik, uint32_t* __restrict__ hist) {
  if (blockIdx.x == 0)  // the select's histograms (its passes are later launches)
    for (int j = threadIdx.x; j < TOPK_HIST_WORDS; j += 256) hist[j] = 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Nc) return;
  const LrIv v = lr_s_interval(grp_ln_interval(el[i], negl != 0), grp_ln_interval(eg[i], negg != 0));
  float l = -INFINITY, h = INFINITY;  // forced: always listed, never lowers U_k
  if (v.kind == LR_IV_NAN) l = NAN;
  if (v.kind == LR_IV_OK) {
    l = v.slo;
    h = v.shi;  // (+inf where g may be 0)
  }
  lo[i] = l;
  hik[i] = hbx_f2ord(h);
}

__global__ __launch_bounds__(TOPK_T) void topk_final_lr_kernel(
    const int32_t* __restrict__ list, const int32_t* __restrict__ count, const double* __restrict__ exact_l,
    const double* __restrict__ exact_g, const double* __restrict__ L, const double* __restrict__ bnd,
    const float* __restrict__ lo, const int32_t* __restrict__ flags, int64_t index_base, int32_t k,
    const KdeParams* __restrict__ Pg, const KdeParams* __restrict__ Pb, const KdeEst* __restrict__ el,
    const KdeEst* __restrict__ eg, TopkHead* __restrict__ head, TopkRec* __restrict__ rec, int32_t* __restrict__ stat) {
  __shared__ uint64_t sk[TOPK_CAP];
  __shared__ int32_t si[TOPK_CAP];
  __shared__ int32_t sp[TOPK_CAP];
  __shared__ int32_t swc[TOPK_T / 64];
  __shared__ int32_t nls, nforce;
  const int t = threadIdx.x;
  const int cnt = *count;
  if (t == 0) nls = nforce = 0;
  __syncthreads();
  auto score = [&](int p) { return L[2 * p + 1] - L[2 * p]; };
  // the absolute bound of one entry's s: both exact pdfs' relative bounds (hbx_acq_impl.h) and the log-space bounds
  auto rel = [&](int p, int32_t idx) { return score_rel(Pg, Pb, el, eg, idx) + bnd[2 * p] + bnd[2 * p + 1]; };
  TopkRank<TOPK_T> rank;
  rank.init(sk, si, sp, swc, TOPK_CAP, k + 1);  // the k best and the best excluded one (the near-tie test's last pair)
  int32_t ls = 0, nf = 0;
  for (int base = 0; base < cnt; base += TOPK_T) {
    const int p = base + t;
    bool acc = false;
    uint64_t key = 0;
    int32_t idx = 0;
    if (p < cnt) {
      key = hbx_d2ord(score(p));
      idx = list[p];
      acc = key != ~0ull && rank.enters(key, idx);  // NaN is never returned
      ls += (bnd[2 * p] > 0.0 ? 1 : 0) + (bnd[2 * p + 1] > 0.0 ? 1 : 0);
      nf += lo[idx] == -INFINITY ? 1 : 0;
    }
    rank.push(acc, key, idx, p);
  }
  rank.finish();
  if (ls) atomicAdd(&nls, ls);
  if (nf) atomicAdd(&nforce, nf);
  const int nb = rank.nb;
  const int nout = nb < k ? nb : k;
  bool near = false;
  for (int j = t; j < nout; j += TOPK_T) {
    const int32_t idx = si[j], p = sp[j];
    const double s = score(p), r = rel(p, idx);
    TopkRec o;
    o.index = (int64_t)idx + index_base;
    o.score = s;
    o.pdf_l = exact_l[p];
    o.pdf_g = exact_g[p];
    o.rel = (float)r;
    o.pad = 0;
    rec[j] = o;
    if (j + 1 < nb) {
      const double w = 1.0001 * (r + rel(sp[j + 1], si[j + 1]));
      near = near || w == INFINITY || score(sp[j + 1]) <= s + w;
    }
  }
  const int any_near = __syncthreads_or(near);
  if (t == 0) {
    TopkHead hd;
    hd.count = nout;
    hd.shortlist = cnt;
    hd.flags = *flags | (any_near ? HBX_ACQ_NEAR_TIE : 0) | HBX_ACQ_LOG_RATIO;
    hd.k = k;
    *head = hd;
    stat[0] = nls;  // (the shortlist's log-space evaluations and forced candidates, as kde_final_lr_kernel leaves them)
    stat[1] = nforce;
  }
}

extern "C" {

int64_t hbx_kde_topk_lr_workspace_bytes(int64_t Nc, int32_t k, int64_t nmax) {
  if (Nc < 0 || k < 1 || k > HBX_TOPK_MAX_K) return -1;
  return (int64_t)(ws_layout(Nc, nmax, 1, true).total + 4 * TOPK_HIST_WORDS);
}

int hbx_kde_acquire_topk_lr(const double* cand, int64_t Nc, int32_t k, int64_t index_base, const void* pair,
                            void* results, void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_acquire_topk_lr";
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const KdePairRef* pp = acq_pair(who, pair);
  if (!pp) return HBX_ERR_ARG;
  const KdePairRef& p = *pp;
  int rc = acq_check(who, p, cand, Nc, workspace);
  if (rc) return rc;
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, HBX_TOPK_MAX_K);
  if (p.D < 1 || p.D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d", who, p.D);
  const int64_t need = hbx_kde_topk_lr_workspace_bytes(Nc, k, p.nmax);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "workspace too small: %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  const hipStream_t s = (hipStream_t)stream;
  const WsLayout w = ws_layout(Nc, p.nmax, 1, true);
  if (Nc == 0) {  // count = 0 and no launch: a zeroed header, and "did not stage" for hbx_kde_acquire_stats
    HBX_HIP(hipMemsetAsync(results, 0, 16, s));
    HBX_HIP(hipMemsetAsync((char*)workspace + w.stage, 0, 4 * HBX_ST_WORDS, s));
    return HBX_OK;
  }
  AcqPlan plan;
  rc = acq_plan(p, true, &plan, acq_lr_coarse());
  if (rc) return rc;
  const AcqWs a(workspace, w);
  uint32_t* hik = (uint32_t*)a.near;                         // the upper bounds' keys in the near list's place
  uint32_t* hist = (uint32_t*)((char*)workspace + w.total);  // the select's histograms after the argmin's workspace
  // unstaged, no timing events, the rescue pass a launch of its own (acquire_lr_impl's request)
  const ScoreRequest rq{cand, Nc, p.D, nullptr, a.rescue, a.init(), p.nmax, false, s};
  ScoreResult sr;
  rc = acq_score(plan, p, a, rq, 0, &sr);
  if (rc) return rc;
  if (plan.exact_only) {  // no estimates: every candidate re-scored (lo = 0, the flag set), no select
    rc = acq_exact_only_init(Nc, (uint32_t)Nc, a, s);
    if (rc) return rc;
    HBX_HIP(hipMemsetAsync(hist, 0, 4 * TOPK_HIST_WORDS, s));
  } else {
    hipLaunchKernelGGL(topk_bounds_lr_kernel, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, a.el, a.eg, Nc,
                       KdeVariant::decode(p.variant_good).has_neg, KdeVariant::decode(p.variant_bad).has_neg, a.lo, hik,
                       hist);
    HBX_LAUNCH_CHECK();
  }
  rc = hbx_topk_shortlist(a.lo, plan.exact_only ? nullptr : hik, Nc, k, hist, a.U, a.flags, a.list, a.count, a.rescue,
                          TopkEval{}, s);
  if (rc) return rc;
  rc = acq_exact(p, cand, Nc, a, false, true, s);
  if (rc) return rc;
  rc = acq_lr_ln(p, cand, Nc, a, s);
  if (rc) return rc;
  hipLaunchKernelGGL(topk_final_lr_kernel, dim3(1), dim3(TOPK_T), 0, s, a.list, a.count, a.exact_l, a.exact_g, a.lr_L,
                     a.lr_bnd, a.lo, a.flags, index_base, k, p.Pg(), p.Pb(), a.el, a.eg, (TopkHead*)results,
                     (TopkRec*)((char*)results + sizeof(TopkHead)), a.lr_stat);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

}  // extern "C"
