// hbx_staged.hip -- staged scoring of the single argmin acquisition: the good KDE (l) for every candidate, the
// bad KDE (g) only for the candidates that can still win.
//
// BOHB's score is max(1e-8, g) / max(l, 1e-8) (bohb.py:129), so whatever g is, score_i >= 1e-8 / max(l_i, 1e-8):
// l alone bounds a candidate's score from below, and any candidate with both sums bounds the best score from
// above.  A candidate whose l-only lower bound lies above that upper bound cannot win or tie; its walk over the
// bad KDE's observations (85 % of the pairs at BOHB's 15 % split) is work the pick does not need.  Where pdfs are
// near or below 1e-8 -- the normal case at D = 32 -- that is all but a few tens of candidates.
//
// Stages, all on the caller's stream, no host round trip (acq_score_staged):
//   1 score l      the good KDE's coarse 32x32 pair kernel over all candidates (observation splits as in the
//                  fused launch), its first workgroup initialising the acquisition's and the stages' state
//     staged_l     rescue of marked candidates, merge of the splits, [llo, lhi] per candidate (est_interval),
//                  lhi kept in a.lo until the combine overwrites it, Lmax = max llo (ordered-uint atomic max)
//   2 seed         every candidate with lhi >= Lmax - ln 4 joins the seed list (at most the list capacity;
//                  the rest fall through to stage 4); every other candidate's g estimate becomes the marker
//                  "g not evaluated" (err = HBX_EST_NOT_EVAL); NaN-l candidates are never seeded
//   3 score seeds  the bad KDE's list instance (kde_logpdf_h32_list_kernel: candidates through an index list
//                  with a device-side count, observation splits into a compact [split][capacity] area), then
//                  staged_merge: splits merged, scattered to a.eg, U_seed = min over seeds of the score
//                  interval's upper end
//   4 survivors    every unseeded candidate with C - max(lhi, C) <= U_seed (C = ln 1e-8; the shortlist's own
//                  '<=', so ties survive) joins the survivor list and is scored like the seeds (more
//                  survivors than the split capacity: one unsplit launch over the list, scattering itself)
//   5 combine      kde_combine_kernel takes a marked candidate's interval from l alone
//                  (score_interval_l_only: slo = C - max(lhi, C), shi = +inf); everything from there on --
//                  shortlist, exact re-score, final argmin -- is the unstaged path's code.
//
// Why the pick is unchanged.  For a pruned candidate the unstaged path computes
//   slo = max(glo, C) - max(lhi, C) >= C - max(lhi, C) > U_seed >= U,
// U being the minimum of the upper ends over ALL candidates: it was never shortlisted there either, and its
// shi >= slo > U never lowered U.  So U, the shortlist, the exact scores, the strict-'<' first-index pick, the
// near set and rel are the same.  That argument needs only VALID intervals for the evaluated candidates, and
// they are: the same scoring body, whose sums do not depend on the lane or block that holds a candidate.  They
// are not the fused launch's bits where the observation splits differ (list_splits here, obs_splits there: the
// partial sums merge in another order and the merged bound grows per merge), so U and the intervals move
// within their bounds.
// What can differ in the record, all of it about the screen and none about the pick:
//   * the unstaged path always shortlists the segment's first certain 1e-8/1e-8 tie (first1); a pruned
//     candidate's tie status is unknown, so when the best score is below 1 `shortlist` is lower by that one
//     candidate, which cannot win;
//   * a candidate at the very edge of the shortlist (slo within the estimates' rounding of U) can fall on
//     either side when the splits differ;
//   * overflow from g: a pruned candidate must not hide HBX_ACQ_OVERFLOW, so where the bad KDE's largest
//     attainable ln pdf (log_norm + ln n: every term is at most 2^0 after the static bound) comes near the
//     flag's limit (700) U_seed stays +inf and every candidate survives (the guard in staged_merge_kernel).  A
//     coarse bound so wide that ghi alone passes 700 (err = +inf) still sets the flag, and the whole-set
//     re-score, in the unstaged path only;
//   * overflow from l (lhi > 700): both paths set the flag and shortlist every candidate whose slo is not NaN;
//     a pruned certain tie has slo = 0 here where the unstaged path gives it NaN (dropped but for first1), so
//     the staged shortlist is then the longer one.
#include "hbx_acquire.h"

#include <hip/hip_ext.h>

#include "hbx_acq_impl.h"
#include "hbx_rescue_impl.h"

#define STAGED_PT 4  // candidates per thread of the selection kernels (1024 per block: few same-address atomics)
#define HBX_LN4f 1.3862943611198906f

// Rescue + split merge + interval of l: afterwards el[i] is the final estimate (what the unstaged path's rescue
// pass and kde_merge_splits_kernel leave), lhi[i] = the interval's upper end (NaN: l is NaN), Lmax raised.
__global__ __launch_bounds__(256) void staged_l_kernel(KdeEst* __restrict__ el, int64_t Nc, int32_t ns,
                                                       const double* __restrict__ cand, int32_t D,
                                                       const KdeParams* __restrict__ Pl,
                                                       const int32_t* __restrict__ rescue_cnt,
                                                       float* __restrict__ lhi, uint32_t* __restrict__ stage) {
  const int32_t nres = *rescue_cnt;  // markers counted by the scoring launch (a hint: garbage only costs time)
  KdeEst e[STAGED_PT];
  if (ns == 1) {
#pragma unroll
    for (int r = 0; r < STAGED_PT; ++r) {
      const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
      if (i < Nc) e[r] = el[i];
    }
  }
  float best = -INFINITY;
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    if (i >= Nc) continue;
    bool mark = false;
    if (ns > 1) {
      if (nres != 0)
        for (int q = 0; q < ns; ++q) mark = mark || el[(int64_t)q * Nc + i].err == -1.f;
      if (!mark) e[r] = merge_splits(el, Nc, i, ns);
    } else {
      mark = e[r].err == -1.f;
    }
    if (mark) e[r] = kde_rescue_one<0, false, true>(cand, i, D, Pl);
    if (ns > 1 || mark) el[i] = e[r];
    float lo, hi = NAN, pt;
    if (e[r].lpos == e[r].lpos) {
      est_interval(e[r], &lo, &hi, &pt);
      best = fmaxf(best, lo);
    }
    lhi[i] = hi;
  }
  __shared__ float rb[4];
  for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
  if ((threadIdx.x & 63) == 0) rb[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float b = fmaxf(fmaxf(rb[0], rb[1]), fmaxf(rb[2], rb[3]));
    const uint32_t o = hbx_f2ord(b);
    if (o > __hip_atomic_load(stage + HBX_ST_LMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(stage + HBX_ST_LMAX, o);
  }
}

// A block's list slots for its flagged candidates: n of this thread; returns the thread's first slot.  One
// atomic per block (same-address atomics serialise in the L2); the list's order is not deterministic and
// nothing downstream depends on it.  Called by every thread of the block.
__device__ __forceinline__ int32_t staged_reserve(int n, int32_t* __restrict__ count) {
  __shared__ int32_t wtot[4];
  __shared__ int32_t base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = n;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  int woff = 0, total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wv) woff += wtot[w];
    total += wtot[w];
  }
  if (threadIdx.x == 0) base = total > 0 ? atomicAdd(count, total) : 0;
  __syncthreads();
  return base + woff + incl - n;
}

// Seeds: lhi >= Lmax - ln 4, up to cap.  A seeded candidate's lhi becomes NaN (stage 4 skips it); every other
// candidate's g estimate becomes the marker.
__global__ __launch_bounds__(256) void staged_seed_kernel(float* __restrict__ lhi, int64_t Nc,
                                                          KdeEst* __restrict__ eg, int32_t* __restrict__ seeds,
                                                          int32_t cap, uint32_t* __restrict__ stage) {
  const float thr = hbx_ord2f(stage[HBX_ST_LMAX]) - HBX_LN4f;
  bool f[STAGED_PT];
  int n = 0;
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    f[r] = false;
    if (i < Nc) {
      const float h = lhi[i];
      f[r] = h == h && h >= thr;
    }
    n += f[r] ? 1 : 0;
  }
  int32_t off = staged_reserve(n, (int32_t*)stage + HBX_ST_NSEED);
  const KdeEst none = {0.f, -INFINITY, HBX_EST_NOT_EVAL, 0.f};
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    if (i >= Nc) continue;
    bool seeded = false;
    if (f[r]) {
      if (off < cap) {
        seeds[off] = (int32_t)i;
        seeded = true;
      }
      ++off;
    }
    if (seeded) lhi[i] = NAN;
    else eg[i] = none;
  }
}

// The list launch's split partials merged and scattered to eg (a marker in any partial: the marker, which the
// combine kernel rescues); update_u: U_seed lowered to the listed candidates' upper score bounds.  Nothing to
// do when the launch ran unsplit over more than cap candidates (it scattered itself).
__global__ __launch_bounds__(256) void staged_merge_kernel(const KdeEst* __restrict__ part, int32_t cap, int32_t ns,
                                                           const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ count, int32_t maxcount,
                                                           const KdeEst* __restrict__ el, KdeEst* __restrict__ eg,
                                                           const KdeParams* __restrict__ Pb,
                                                           uint32_t* __restrict__ stage, int32_t update_u) {
  int32_t cnt = *count;
  if (cnt > maxcount) cnt = maxcount;
  if (cnt > cap) return;
  const int32_t k = blockIdx.x * 256 + threadIdx.x;
  float h = INFINITY;
  if (k < cnt) {
    const int32_t i = idx[k];
    bool mark = false;
    for (int q = 0; q < ns; ++q) mark = mark || part[(int64_t)q * cap + k].err == -1.f;
    KdeEst e = {0.f, -INFINITY, -1.f, 0.f};
    if (!mark) e = merge_splits(part, cap, k, ns);
    eg[i] = e;
    if (update_u && !mark) {
      const ScoreIv v = score_interval(el[i], e);
      if (!v.lnan) h = v.shi;
    }
  }
  if (update_u) {
    // overflow guard (file header): no pruning when the bad KDE's ln pdf can come near the flag's limit
    const bool guard = Pb->log_norm + log((double)(Pb->n > 1 ? Pb->n : 1)) < 600.0;
    for (int o = 32; o > 0; o >>= 1) h = fminf(h, __shfl_xor(h, o));
    if ((threadIdx.x & 63) == 0 && guard && h < INFINITY) {
      const uint32_t o = hbx_f2ord(h);
      if (o < __hip_atomic_load(stage + HBX_ST_USEED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(stage + HBX_ST_USEED, o);
    }
  }
}

// Survivors: unseeded, l not NaN, l-only lower score bound <= U_seed.
__global__ __launch_bounds__(256) void staged_survivor_kernel(const float* __restrict__ lhi, int64_t Nc,
                                                              int32_t* __restrict__ surv,
                                                              uint32_t* __restrict__ stage) {
  const float U = hbx_ord2f(stage[HBX_ST_USEED]);
  const float C = (float)HBX_LN_CLAMP;
  bool f[STAGED_PT];
  int n = 0;
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    f[r] = false;
    if (i < Nc) {
      const float h = lhi[i];
      f[r] = h == h && (C - fmaxf(h, C)) <= U;
    }
    n += f[r] ? 1 : 0;
  }
  int32_t off = staged_reserve(n, (int32_t*)stage + HBX_ST_NSURV);
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    if (i < Nc && f[r]) surv[off++] = (int32_t)i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) stage[HBX_ST_FLAG] = 1;  // this call staged (hbx_kde_acquire_stats)
}

// ------------------------------------------------------------------------------------------
// launch side

bool acq_staged_supported(const AcqPlan& plan) {
  return HBX_PAIR_INIT && !plan.exact_only && plan.fg.list && plan.fb.list && plan.fg.pair && plan.fg.split_ok;
}

int acq_score_staged(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                     hipEvent_t* ev, hipStream_t s) {
  // stage 1: the good KDE's pair kernel with every block in its first segment; the good KDE has the chip's block
  // slots to itself (pair_shape's kdes = 1)
  const ScoreFns& f = plan.fg;
  const PairShape sh = pair_shape(f, true, 1, Nc, p.nmax);
  const int ns = sh.nsplit;
  const unsigned grid = sh.tiles * (unsigned)ns;
  KdePairArgs ka{p.Pg(), p.Pg(), p.table_good, p.table_good, a.el, a.el, grid, a.rescue, a.init()};
  ka.tiles = sh.tiles;
  ka.nsplit0 = ka.nsplit1 = ns;
  ka.row_stage = hbx_row_stage();
  if (ev)  // stamped by the dispatch at the kernel's start
    hipExtLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, ev[0], nullptr, 0, cand, Nc, p.D, ka);
  else
    hipLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, cand, Nc, p.D, ka);
  HBX_LAUNCH_CHECK();
  const dim3 gsel((unsigned)((Nc + 256 * STAGED_PT - 1) / (256 * STAGED_PT)));
  hipLaunchKernelGGL(staged_l_kernel, gsel, dim3(256), 0, s, a.el, Nc, (int32_t)ns, cand, p.D, p.Pg(), a.rescue, a.lo,
                     a.stage);
  HBX_LAUNCH_CHECK();
  // stage 2
  const int32_t cap = a.list_cap;
  hipLaunchKernelGGL(staged_seed_kernel, gsel, dim3(256), 0, s, a.lo, Nc, a.eg, a.seeds, cap, a.stage);
  HBX_LAUNCH_CHECK();
  // stage 3
  const ScoreFns& fb = plan.fb;
  const int ls = list_splits(p.nmax);
  const unsigned tcap = (unsigned)(cap / fb.cands_per_block);
  KdeListArgs la{p.Pb(), p.table_bad, a.eg, a.lpart, a.seeds, (const int32_t*)a.stage + HBX_ST_NSEED, a.rescue, cap,
                 cap, ls, tcap, ka.row_stage};
  hipLaunchKernelGGL(fb.list, dim3(tcap * (unsigned)ls), dim3(fb.threads), 0, s, cand, p.D, la);
  HBX_LAUNCH_CHECK();
  const dim3 gmerge((unsigned)((cap + 255) / 256));
  hipLaunchKernelGGL(staged_merge_kernel, gmerge, dim3(256), 0, s, a.lpart, cap, (int32_t)ls, a.seeds, la.count, cap,
                     a.el, a.eg, p.Pb(), a.stage, 1);
  HBX_LAUNCH_CHECK();
  // stage 4
  hipLaunchKernelGGL(staged_survivor_kernel, gsel, dim3(256), 0, s, a.lo, Nc, a.surv, a.stage);
  HBX_LAUNCH_CHECK();
  la.idx = a.surv;
  la.count = (const int32_t*)a.stage + HBX_ST_NSURV;
  la.maxcount = (int32_t)Nc;
  const unsigned gfull = (unsigned)((Nc + fb.cands_per_block - 1) / fb.cands_per_block);
  const unsigned gsplit = tcap * (unsigned)ls;
  hipLaunchKernelGGL(fb.list, dim3(gfull > gsplit ? gfull : gsplit), dim3(fb.threads), 0, s, cand, p.D, la);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(staged_merge_kernel, gmerge, dim3(256), 0, s, a.lpart, cap, (int32_t)ls, a.surv, la.count,
                     (int32_t)Nc, a.el, a.eg, p.Pb(), a.stage, 0);
  HBX_LAUNCH_CHECK();
  if (ev) {  // [0]->[1]: the staged scoring, first launch's start to the last launch's end
    HBX_HIP(hipEventRecord(ev[1], s));
    HBX_HIP(hipEventRecord(ev[2], s));
  }
  return HBX_OK;
}

extern "C" {

// What the last single acquisition on this workspace did (device read, synchronises): out[0] = 1 when it
// staged, [1] seeds, [2] survivors, [3] candidates whose g was evaluated (Nc when it did not stage).
int hbx_kde_acquire_stats(const void* workspace, int64_t Nc, int64_t nmax, int64_t* out) {
  if (!workspace || !out || Nc < 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_acquire_stats: bad arguments");
  const WsLayout w = ws_layout(Nc, nmax);
  uint32_t st[HBX_ST_WORDS];
  HBX_HIP(hipDeviceSynchronize());
  HBX_HIP(hipMemcpy(st, (const char*)workspace + w.stage, sizeof(st), hipMemcpyDeviceToHost));
  const bool staged = st[HBX_ST_FLAG] == 1;
  const int64_t seeds = staged ? ((int64_t)st[HBX_ST_NSEED] < w.list_cap ? (int64_t)st[HBX_ST_NSEED] : w.list_cap) : 0;
  const int64_t surv = staged ? (int64_t)st[HBX_ST_NSURV] : 0;
  out[0] = staged ? 1 : 0;
  out[1] = seeds;
  out[2] = surv;
  out[3] = staged ? seeds + surv : Nc;
  return HBX_OK;
}

}  // extern "C"
