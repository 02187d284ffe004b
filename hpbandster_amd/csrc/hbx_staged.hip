// hbx_staged.hip -- staged scoring of the single argmin acquisition: the good KDE (l) for every candidate, the
// bad KDE (g) only for the candidates that can still win.
//
// BOHB's score is max(f, g) / max(l, f) (bohb.py:129; f: the pair's score floor, the reference's 1e-8 unless set: every
// argument below is stated in C = ln f and holds for any f), so whatever g is, score_i >= f / max(l_i, f):
// l alone bounds a candidate's score from below, and any candidate with both sums bounds the best score from
// above.  A candidate whose l-only lower bound lies above that upper bound cannot win or tie; its walk over the
// bad KDE's observations (85 % of the pairs at BOHB's 15 % split) is work the pick does not need.  Where pdfs are
// near or below f -- at the reference's 1e-8 the normal case at D = 32 -- that is all but a few tens of candidates.
//
// Stages, all on the caller's stream, no host round trip (acq_score_staged):
//   1 score l      the good KDE's coarse 32x32 pair kernel over all candidates (observation splits as in the
//                  fused launch), its first workgroup initialising the acquisition's and the stages' state
//                  Unsplit (pair_shape's nsplit = 1; the bench's size): the kernel's epilogue, which holds each
//                  candidate's finished estimate in a register, also leaves [llo, lhi] (est_interval) -- lhi in
//                  a.lo, kept until stage 4 / 5 overwrites it, and per block the largest llo in a.bmax, an area
//                  of its own in the workspace (4 bytes per 256 candidates; not an alias of the split partials,
//                  so no block count at which this would have to be off).  No atomic, and nothing that races the
//                  first workgroup's initialisation.  A rescue-marked candidate cannot be re-scored there: its lhi
//                  is +inf and it contributes nothing to its block's maximum.  KdePairArgs::lhi / bmax.
//     staged_l     a launch of its own where stage 1 ran split (partials to merge), for the staged top-k (KEYS)
//                  and under HBX_STAGE1_LHI=0 (tests, A/B): rescue of marked candidates, merge of the splits,
//                  [llo, lhi] per candidate, lhi into a.lo, Lmax = max llo (ordered-uint atomic max)
//   2 seed         every candidate with lhi >= Lmax - ln 4 joins the seed list (at most the list capacity;
//                  the rest fall through to stage 4); NaN-l candidates are never seeded.  Behind the epilogue's
//                  lhi, every block of the seed kernel first reduces the block maxima to Lmax itself (1954
//                  floats on the bench; block 0 stores it in the state words for hbx_kde_acquire_stats and the
//                  tools), and a candidate whose lhi reads +inf is looked up: a rescue marker is re-scored here
//                  (kde_rescue_one, staged_l's call), its estimate stored, its interval's upper end taken as lhi
//                  and tested like any other.  Lmax is then the largest llo over the UNMARKED candidates: lower
//                  than staged_l's or equal, so the seed set can only grow.  The pick does not depend on which
//                  candidates are seeds -- only U_seed and the survivor criterion enter the argument below, and
//                  both hold for any seed set -- so only the seed and survivor counts can differ between the two
//                  forms, and only where l estimates are marked.  (HBX_STAGED_TAIL=0:
//                  every other candidate's g estimate becomes the marker "g not evaluated", err =
//                  HBX_EST_NOT_EVAL, for the combine kernel)
//   3 score seeds  the bad KDE's list instance (kde_logpdf_h32_list_kernel: candidates through an index list
//                  with a device-side count, observation splits into a compact [split][capacity] area), then
//                  staged_merge: splits merged, scattered to a.eg, U_seed = min over seeds of the score
//                  interval's upper end
//   4 survivors    every unseeded candidate with C - max(lhi, C) <= U_seed (C = ln f; the shortlist's own
//                  '<=', so ties survive) joins the survivor list and is scored like the seeds (more
//                  survivors than the split capacity: one unsplit launch over the list, scattering itself).
//                  The same pass turns every unseeded candidate's a.lo entry from lhi into its l-only lower
//                  score bound C - max(lhi, C) (score_interval_l_only's slo; NaN stays NaN) and raises the
//                  overflow flag where lhi > 700: a pruned candidate's whole contribution to what follows
//   5 tail         staged_tail_kernel, over the evaluated candidates only (seeds and survivors): the
//                  survivors' partials merged and scattered, marked g estimates re-scored, score_interval as
//                  the combine kernel computes it -> a.lo, U, first1, the flag, and a preliminary shortlist
//                  against an upper bound of U; staged_shortlist_kernel (one block) filters that list with
//                  the final U.  No pass over all candidates, and nothing reads the g estimate of an
//                  unevaluated candidate (the final kernel's score_rel takes it only for a signed KDE, and
//                  staged pairs are unsigned), so the marker is not written.  Then the unstaged path's exact
//                  re-score and final argmin.
//                  HBX_STAGED_TAIL=0 (tests, A/B): the earlier sequence instead -- the survivors' merge, then
//                  kde_combine_kernel over all candidates (a marked candidate's interval from l alone) and
//                  kde_shortlist_kernel over all candidates.  Same functions, same operands: same bits.
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
//   * the unstaged path always shortlists the segment's first certain f/f tie (first1); a pruned
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
// blocks at most of the seed kernel behind stage 1's epilogue: every block reads every block maximum (Nc / 512
// floats), so an unbounded grid would read Nc^2 / 2^19 floats -- 760 MB at 1e7 candidates, more than staged_l_kernel
// moved; 2048 blocks (two rounds of the chip at 4 blocks per CU) keep it at 160 MB there and change nothing
// below 2.1e6 candidates
#define STAGED_SEED_BLOCKS 2048

// Rescue + split merge + interval of l: afterwards el[i] is the final estimate (what the unstaged path's rescue
// pass and kde_merge_splits_kernel leave), lhi[i] = the interval's upper end (NaN: l is NaN), Lmax raised.
// KEYS (the staged top-k, hbx_topk.hip): also lkey[i] = the ordered key of -llo (+inf: l is NaN or llo = -inf), for the
// radix select of the (k+1)-th largest llo, whose histograms (hist_words words) the first block zeroes.
template <bool KEYS>
__global__ __launch_bounds__(256) void staged_l_kernel(KdeEst* __restrict__ el, int64_t Nc, int32_t ns,
                                                       const double* __restrict__ cand, int32_t D,
                                                       const KdeParams* __restrict__ Pl,
                                                       const int32_t* __restrict__ rescue_cnt,
                                                       float* __restrict__ lhi, uint32_t* __restrict__ stage,
                                                       uint32_t* __restrict__ lkey, uint32_t* __restrict__ hist,
                                                       int32_t hist_words) {
  if constexpr (KEYS) {
    if (blockIdx.x == 0)
      for (int j = threadIdx.x; j < hist_words; j += 256) hist[j] = 0;
  }
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
    float lo = -INFINITY, hi = NAN, pt;
    if (e[r].lpos == e[r].lpos) {
      est_interval(e[r], &lo, &hi, &pt);
      best = fmaxf(best, lo);
    }
    lhi[i] = hi;
    if constexpr (KEYS) lkey[i] = hbx_f2ord(-lo);
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

// Seeds: lhi >= Lmax - ln 4, up to cap.  A seeded candidate's lhi becomes NaN (stage 4 skips it); mark_rest (the
// combine kernel follows): every other candidate's g estimate becomes the marker.
// bmax (stage 1's epilogue left lhi; null: Lmax is in the state words): Lmax is the largest of the nblk block maxima,
// which every block reduces for itself (a float per 256 or 512 candidates, from the L2), block 0 storing it and
// the fold's flag in the state words; and a candidate whose lhi reads +inf is looked up in el: a rescue marker is
// re-scored here as staged_l_kernel does it, its estimate stored and its interval's upper end taken for lhi.
__global__ __launch_bounds__(256) void staged_seed_kernel(float* __restrict__ lhi, int64_t Nc,
                                                          KdeEst* __restrict__ eg, int32_t* __restrict__ seeds,
                                                          int32_t cap, uint32_t* __restrict__ stage,
                                                          int32_t mark_rest, const float* __restrict__ bmax,
                                                          int32_t nblk, const double* __restrict__ cand, int32_t D,
                                                          const KdeParams* __restrict__ Pl,
                                                          KdeEst* __restrict__ el) {
  float lmax;
  if (bmax) {  // (uniform)
    __shared__ float rb[4];
    float m = -INFINITY;
    // 16-byte loads, four per thread in flight (4096 maxima a round: one round up to 1e6 candidates), the area being
    // 256-byte aligned in the workspace like every other (ws_layout); then the last nblk % 4.  The maximum does not
    // depend on the order it is taken in (no NaN among the block maxima, and no -0: est_interval's lo)
    const float4* b4 = (const float4*)bmax;
    const int n4 = nblk >> 2;
    for (int j = threadIdx.x; j < n4; j += 4 * 256) {
      float4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        v[q] = j + q * 256 < n4 ? b4[j + q * 256] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
      for (int q = 0; q < 4; ++q) m = fmaxf(m, fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w)));
    }
    for (int j = (n4 << 2) + threadIdx.x; j < nblk; j += 256) m = fmaxf(m, bmax[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) rb[threadIdx.x >> 6] = m;
    __syncthreads();
    lmax = fmaxf(fmaxf(rb[0], rb[1]), fmaxf(rb[2], rb[3]));
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // for hbx_kde_acquire_stats / _stage1 and the tools
      stage[HBX_ST_LMAX] = hbx_f2ord(lmax);
      stage[HBX_ST_LHI1] = 1;
    }
  } else {
    lmax = hbx_ord2f(stage[HBX_ST_LMAX]);
  }
  const float thr = lmax - HBX_LN4f;
  // a block takes the 1024-candidate tiles blockIdx.x, + gridDim.x, ...: one tile each up to STAGED_SEED_BLOCKS
  // tiles; the grid stops growing there, so that the blocks' reads of the block maxima do (staged_score_seeds)
  const int64_t ntile = (Nc + 256 * STAGED_PT - 1) / (256 * STAGED_PT);
  for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
  bool f[STAGED_PT];
  int n = 0;
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = (tb * STAGED_PT + r) * 256 + threadIdx.x;
    f[r] = false;
    if (i < Nc) {
      float h = lhi[i];
      if (bmax && h == INFINITY) {  // rare: stage 1 marked the candidate (or its bound is +inf itself)
        KdeEst e = el[i];
        if (e.err == -1.f) {
          e = kde_rescue_one<0, false, true>(cand, i, D, Pl);
          el[i] = e;
          float lo, pt;
          h = NAN;
          if (e.lpos == e.lpos) est_interval(e, &lo, &h, &pt);
          lhi[i] = h;
        }
      }
      f[r] = h == h && h >= thr;
    }
    n += f[r] ? 1 : 0;
  }
  int32_t off = staged_reserve(n, (int32_t*)stage + HBX_ST_NSEED);
  const KdeEst none = {0.f, -INFINITY, HBX_EST_NOT_EVAL, 0.f};
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = (tb * STAGED_PT + r) * 256 + threadIdx.x;
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
    else if (mark_rest) eg[i] = none;  // (uniform; the short tail reads no g estimate of an unevaluated candidate)
  }
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
                                                           uint32_t* __restrict__ stage, int32_t update_u,
                                                           ScoreFloor F) {
  int32_t cnt = *count;
  if (cnt > maxcount) cnt = maxcount;
  if (cnt > cap) return;
  const int32_t k = blockIdx.x * 256 + threadIdx.x;
  float h = INFINITY;
  if (k < cnt) {
    const int32_t i = idx[k];
    // the ns partials and the l estimate requested together; the marker test and the merge on the loaded partials
    const KdeEst a = update_u ? el[i] : kde_est_neutral();
    bool mark;
    const KdeEst e = merge_splits_or_marker(part, cap, k, ns, &mark);
    eg[i] = e;
    if (update_u && !mark) {
      const ScoreIv v = score_interval(a, e, F);
      if (!v.lnan) h = v.shi;
    }
  }
  if (update_u) {
    // overflow guard (file header): no pruning when the bad KDE's ln pdf can come near the flag's limit; the test
    // log_norm + ln n < 600 is made once per KDE where its parameters are written (KdeParams::lnpdf_guard)
    const bool guard = Pb->lnpdf_guard != 0;
    for (int o = 32; o > 0; o >>= 1) h = fminf(h, __shfl_xor(h, o));
    if ((threadIdx.x & 63) == 0 && guard && h < INFINITY) {
      const uint32_t o = hbx_f2ord(h);
      if (o < __hip_atomic_load(stage + HBX_ST_USEED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(stage + HBX_ST_USEED, o);
    }
  }
}

// Survivors: unseeded, l not NaN, l-only lower score bound <= U_seed.
// flags (the short tail; null: the combine kernel follows): lhi[i], which is a.lo, becomes the l-only interval's
// lower end C - max(lhi, C) (less F.w) in place -- score_interval_l_only's slo from the same lhi -- NaN staying NaN (l is NaN,
// or a seed, whose entry the tail kernel writes), and lhi > 700 raises the overflow flag as that interval's `of`.
__global__ __launch_bounds__(256) void staged_survivor_kernel(float* __restrict__ lhi, int64_t Nc,
                                                              int32_t* __restrict__ surv,
                                                              uint32_t* __restrict__ stage,
                                                              int32_t* __restrict__ flags, ScoreFloor F) {
  const float U = hbx_ord2f(stage[HBX_ST_USEED]);
  const float C = F.C;
  bool f[STAGED_PT];
  int n = 0;
#pragma unroll
  for (int r = 0; r < STAGED_PT; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * STAGED_PT + r) * 256 + threadIdx.x;
    f[r] = false;
    if (i < Nc) {
      const float h = lhi[i];
      f[r] = h == h && (C - fmaxf(h, C) - F.w) <= U;
      if (flags && h == h) {  // (flags: uniform)
        lhi[i] = C - fmaxf(h, C) - F.w;
        if (h > 700.f) atomicOr(flags, 1);
      }
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

// The short tail (HBX_STAGED_TAIL): what the second merge, the combine and the shortlist launches did, in two
// launches over the evaluated candidates only -- the seeds (their g estimates merged and scattered by the first merge) and the
// survivors (their split partials merged here; an unsplit survivor launch scattered its own).  Every other
// candidate's interval is a function of lhi alone and the survivor pass has written it.
struct StagedTailArgs {
  const KdeEst* part;  // the survivor launch's split partials [ns][cap]
  int32_t cap, ns;
  const int32_t* seeds;
  const int32_t* surv;
  int64_t Nc;
  const double* cand;
  int32_t D;
  const KdeParams* Pb;
  const KdeEst* el;
  KdeEst* eg;
  float* lo;
  uint32_t* U;
  int32_t* flags;
  int32_t* first1;
  int32_t* list;
  int32_t* count;
  int32_t* rescue_cnt;
  uint32_t* stage;
  ScoreFloor F;
};

// agent-scope loads of words other blocks of the same launch lower (never through the scalar or a stale vector cache)
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t ld_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entry k of the evaluated candidates (seeds first, then survivors); a block owns 1024 consecutive entries, TAIL_PT
// per thread (their loads in flight together, their indices and lower bounds kept in registers), and the blocks
// past the last entry exit at once:
//   1  its g estimate: merged from the partials (a marker in any: the marker) or as scattered; a marked one
//      re-scored (kde_rescue_one, the RESCUE combine's call) and stored; score_interval(el, eg) as the combine
//      computes it: lo[i] (NaN for a certain tie), U, first1 and the overflow flag lowered / raised per wave, an
//      atomic only where it changes the value
//   2  the preliminary shortlist: its entries with lo <= u, u an upper bound of the final U (U only falls: U_seed,
//      and U as read after the block's atomics), and each certain tie that lowered first1; slots by one atomic
//      per block.  The final U is known only when every block has run: staged_shortlist_kernel.
// (Measured, profiles/staged_tail: one launch for both -- a fence and a ticket per block, the last block to
// finish filtering -- takes 76-97 us where every one of 1e6 candidates is evaluated, against 26 us for the three
// launches it replaced; the device-scope release of each of its blocks is what costs.  Two launches need none.)
#define TAIL_THREADS 1024  // of the one-block shortlist kernel
#define TAIL_PT 4
__global__ __launch_bounds__(256) void staged_tail_kernel(StagedTailArgs t) {
  constexpr int TAIL_THREADS_A = 256;
  constexpr int NW = TAIL_THREADS_A / 64;
  __shared__ int32_t swc[NW];
  __shared__ uint32_t pbase;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t nseed = (int32_t)t.stage[HBX_ST_NSEED], nsurv = (int32_t)t.stage[HBX_ST_NSURV];
  if (nseed > t.cap) nseed = t.cap;
  if (nsurv > t.Nc) nsurv = t.Nc;
  const bool split = nsurv <= t.cap;  // else the unsplit launch scattered its estimates itself
  const int64_t total = nseed + nsurv;
  constexpr int64_t EPB = (int64_t)TAIL_PT * TAIL_THREADS_A;
  const int64_t nwork = (total + EPB - 1) / EPB;  // (<= the grid, sized for Nc + cap entries)
  if (blockIdx.x >= nwork) return;  // no entries
  const int32_t nres = *t.rescue_cnt;  // markers counted by the scoring launches (a hint, as in the combine)
  // 1
  int32_t idx[TAIL_PT];
  KdeEst ea[TAIL_PT], eb[TAIL_PT];
  float slo[TAIL_PT];
#pragma unroll
  for (int r = 0; r < TAIL_PT; ++r) {
    const int64_t k = (int64_t)blockIdx.x * EPB + r * TAIL_THREADS_A + threadIdx.x;
    idx[r] = -1;
    if (k < total) idx[r] = k < nseed ? t.seeds[k] : t.surv[k - nseed];
  }
#pragma unroll
  for (int r = 0; r < TAIL_PT; ++r) {
    const int64_t k = (int64_t)blockIdx.x * EPB + r * TAIL_THREADS_A + threadIdx.x;
    if (idx[r] < 0) continue;
    ea[r] = t.el[idx[r]];
    if (k < nseed || !split) eb[r] = t.eg[idx[r]];
  }
  float h = INFINITY;
  int32_t f1 = INT32_MAX;
  bool of = false;
#pragma unroll
  for (int r = 0; r < TAIL_PT; ++r) {
    const int64_t k = (int64_t)blockIdx.x * EPB + r * TAIL_THREADS_A + threadIdx.x;
    slo[r] = NAN;
    if (idx[r] < 0) continue;
    const int64_t i = idx[r];
    bool store = false;
    if (!(k < nseed || !split)) {
      const int64_t ks = k - nseed;
      bool mark;
      eb[r] = merge_splits_or_marker(t.part, t.cap, ks, t.ns, &mark);
      store = true;
    }
    if (nres != 0 && eb[r].err == -1.f) {  // rare
      eb[r] = kde_rescue_one<0, false, true>(t.cand, i, t.D, t.Pb);
      store = true;
    }
    if (store) t.eg[i] = eb[r];
    const ScoreIv v = score_interval(ea[r], eb[r], t.F);
    slo[r] = v.one ? NAN : v.slo;
    t.lo[i] = slo[r];
    if (!v.lnan) h = fminf(h, v.shi);
    if (v.one && (int32_t)i < f1) f1 = (int32_t)i;
    of = of || v.of;
  }
  float hw = h;
  int32_t fw = f1;
  for (int o = 32; o > 0; o >>= 1) {
    hw = fminf(hw, __shfl_xor(hw, o));
    fw = min(fw, __shfl_xor(fw, o));
  }
  const bool ofw = __ballot(of) != 0;
  bool lowered = false;  // lane 0: the wave's first certain tie lowered first1
  if (lane == 0) {
    const uint32_t o = hbx_f2ord(hw);
    if (hw < INFINITY && o < ld_agent(t.U)) atomicMin(t.U, o);
    if (fw != INT32_MAX && fw < ld_agent(t.first1)) lowered = atomicMin(t.first1, fw) > fw;
    if (ofw) atomicOr(t.flags, 1);
  }
  lowered = __shfl(lowered ? 1 : 0, 0) != 0;
  // 2 (behind a barrier: U has this block's minima, and those of the blocks that run at its pace)
  __syncthreads();
  const float useed = hbx_ord2f(t.stage[HBX_ST_USEED]);  // (final since the first merge)
  const float u = fminf(useed, hbx_ord2f(ld_agent(t.U)));
  int n = 0;
#pragma unroll
  for (int r = 0; r < TAIL_PT; ++r) {
    const float l = slo[r];
    if (!(idx[r] >= 0 && ((l == l && l <= u) || (lowered && idx[r] == fw)))) idx[r] = -1;
    n += idx[r] >= 0 ? 1 : 0;
  }
  {  // the block's slots: one atomic per block, as staged_reserve
    int incl = n;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) swc[wv] = incl;
    __syncthreads();
    int off = incl - n, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      off += w < wv ? swc[w] : 0;
      tot += swc[w];
    }
    if (threadIdx.x == 0) pbase = tot > 0 ? atomicAdd(t.stage + HBX_ST_NPRE, (uint32_t)tot) : 0u;
    __syncthreads();
    off += (int)pbase;
#pragma unroll
    for (int r = 0; r < TAIL_PT; ++r)
      if (idx[r] >= 0) t.list[off++] = idx[r];
  }
}

// ... and the shortlist from the preliminary one, by one block behind the launch above (every interval is stored, U,
// first1 and the flag are final): the entries with lo <= U or the index first1, compacted in place
// (kde_shortlist_kernel's predicate; a pruned candidate has lo > U_seed >= U).  Overflow flag set: every candidate
// whose lo is not NaN instead (slow; the fp64 re-score of the whole set behind it dominates).  It zeroes the marker
// count for the next call, as the shortlist kernel does.
__global__ __launch_bounds__(TAIL_THREADS) void staged_shortlist_kernel(StagedTailArgs t) {
  constexpr int NW = TAIL_THREADS / 64;
  constexpr int64_t EPB = (int64_t)TAIL_PT * TAIL_THREADS;
  __shared__ int32_t swc[NW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t npre = t.stage[HBX_ST_NPRE];
  const float uf = hbx_ord2f(t.U[0]);
  const int32_t ff = t.first1[0];
  const bool all = (t.flags[0] & 1) != 0;
  const int64_t nscan = all ? t.Nc : npre;
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < nscan; c0 += EPB) {  // TAIL_PT consecutive entries per thread: the order is kept
    const int64_t c = c0 + (int64_t)TAIL_PT * threadIdx.x;
    int32_t ci[TAIL_PT];
    float cl[TAIL_PT];
#pragma unroll
    for (int r = 0; r < TAIL_PT; ++r) ci[r] = c + r < nscan ? (all ? (int32_t)(c + r) : t.list[c + r]) : -1;
#pragma unroll
    for (int r = 0; r < TAIL_PT; ++r) cl[r] = ci[r] >= 0 ? t.lo[ci[r]] : NAN;
    int n = 0;
#pragma unroll
    for (int r = 0; r < TAIL_PT; ++r) {
      if (!(ci[r] >= 0 && ((cl[r] == cl[r] && (all || cl[r] <= uf)) || ci[r] == ff))) ci[r] = -1;
      n += ci[r] >= 0 ? 1 : 0;
    }
    int incl = n;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) swc[wv] = incl;
    __syncthreads();  // (and every read of this round's entries before a store: base <= c0, in place)
    int64_t off = base + incl - n;
    int tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      off += w < wv ? swc[w] : 0;
      tot += swc[w];
    }
#pragma unroll
    for (int r = 0; r < TAIL_PT; ++r)
      if (ci[r] >= 0) t.list[off++] = ci[r];
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *t.count = (int32_t)base;
    *t.rescue_cnt = 0;  // (the preliminary list's length stays, like the counts: the next call's first scoring
                        // block zeroes it)
  }
}

// ------------------------------------------------------------------------------------------
// launch side

bool acq_staged_supported(const AcqPlan& plan) {
  return HBX_PAIR_INIT && !plan.exact_only && plan.fg.list && plan.fb.list && plan.fg.pair && plan.fg.split_ok;
}

// the selection kernels' grid: 1024 candidates per block
static dim3 staged_gsel(int64_t Nc) { return dim3((unsigned)((Nc + 256 * STAGED_PT - 1) / (256 * STAGED_PT))); }

// the list launches' arguments: the bad KDE's list instance over the seed list
static KdeListArgs staged_list_args(const AcqPlan& plan, const KdePairRef& p, const AcqWs& a) {
  const int32_t cap = a.list_cap;
  return KdeListArgs{p.Pb(), p.table_bad, a.eg, a.lpart, a.seeds, (const int32_t*)a.stage + HBX_ST_NSEED, a.rescue,
                     cap,    cap,         list_splits(p.nmax), (unsigned)(cap / plan.fb.cands_per_block),
                     hbx_row_stage()};
}

int staged_score_l(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                   hipEvent_t* ev, hipStream_t s, uint32_t* lkey, uint32_t* hist, int32_t hist_words,
                   unsigned* lhi_blocks) {
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
  // the argmin's stage 1, unsplit: lhi and the block maxima from the scoring kernel's epilogue, no staged_l launch.
  // (A split launch has partials to merge, and the staged top-k wants every candidate's key: staged_l_kernel.)
  const bool fold = lhi_blocks && !lkey && ns == 1 && hbx_stage1_lhi();
  if (lhi_blocks) *lhi_blocks = fold ? grid : 0;
  if (fold) {
    ka.lhi = a.lo;
    ka.bmax = a.bmax;  // (one float per block: grid <= ceil(Nc / 256), the area's size)
  }
  if (ev)  // stamped by the dispatch at the kernel's start
    hipExtLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, ev[0], nullptr, 0, cand, Nc, p.D, ka);
  else
    hipLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, cand, Nc, p.D, ka);
  HBX_LAUNCH_CHECK();
  if (fold) return HBX_OK;
  if (lkey)
    hipLaunchKernelGGL(staged_l_kernel<true>, staged_gsel(Nc), dim3(256), 0, s, a.el, Nc, (int32_t)ns, cand, p.D,
                       p.Pg(), a.rescue, a.lo, a.stage, lkey, hist, hist_words);
  else
    hipLaunchKernelGGL(staged_l_kernel<false>, staged_gsel(Nc), dim3(256), 0, s, a.el, Nc, (int32_t)ns, cand, p.D,
                       p.Pg(), a.rescue, a.lo, a.stage, (uint32_t*)nullptr, (uint32_t*)nullptr, 0);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int staged_score_seeds(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                       hipStream_t s, bool mark_rest, bool update_u, unsigned lhi_blocks) {
  // stage 2
  const int32_t cap = a.list_cap;
  dim3 gseed = staged_gsel(Nc);
  if (lhi_blocks && gseed.x > STAGED_SEED_BLOCKS) gseed.x = STAGED_SEED_BLOCKS;
  hipLaunchKernelGGL(staged_seed_kernel, gseed, dim3(256), 0, s, a.lo, Nc, a.eg, a.seeds, cap, a.stage,
                     (int32_t)(mark_rest ? 1 : 0), lhi_blocks ? (const float*)a.bmax : (const float*)nullptr,
                     (int32_t)lhi_blocks, cand, p.D, p.Pg(), a.el);
  HBX_LAUNCH_CHECK();
  // stage 3
  const ScoreFns& fb = plan.fb;
  const KdeListArgs la = staged_list_args(plan, p, a);
  hipLaunchKernelGGL(fb.list, dim3(la.tiles_cap * (unsigned)la.nsplit), dim3(fb.threads), 0, s, cand, p.D, la);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(staged_merge_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, a.lpart, cap,
                     la.nsplit, a.seeds, la.count, cap, a.el, a.eg, p.Pb(), a.stage, (int32_t)(update_u ? 1 : 0),
                     p.floor);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int staged_score_survivors(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                           hipStream_t s, bool lonly) {
  // stage 4
  const ScoreFns& fb = plan.fb;
  hipLaunchKernelGGL(staged_survivor_kernel, staged_gsel(Nc), dim3(256), 0, s, a.lo, Nc, a.surv, a.stage,
                     lonly ? a.flags : (int32_t*)nullptr, p.floor);
  HBX_LAUNCH_CHECK();
  KdeListArgs la = staged_list_args(plan, p, a);
  la.idx = a.surv;
  la.count = (const int32_t*)a.stage + HBX_ST_NSURV;
  la.maxcount = (int32_t)Nc;
  const unsigned gfull = (unsigned)((Nc + fb.cands_per_block - 1) / fb.cands_per_block);
  const unsigned gsplit = la.tiles_cap * (unsigned)la.nsplit;
  hipLaunchKernelGGL(fb.list, dim3(gfull > gsplit ? gfull : gsplit), dim3(fb.threads), 0, s, cand, p.D, la);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int acq_score_staged(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                     hipEvent_t* ev, hipStream_t s, bool tail) {
  unsigned lhi_blocks = 0;
  int rc = staged_score_l(plan, p, cand, Nc, a, ev, s, nullptr, nullptr, 0, &lhi_blocks);
  if (rc) return rc;
  rc = staged_score_seeds(plan, p, cand, Nc, a, s, !tail, true, lhi_blocks);
  if (rc) return rc;
  rc = staged_score_survivors(plan, p, cand, Nc, a, s, tail);
  if (rc) return rc;
  const int32_t cap = a.list_cap;
  const int32_t ls = list_splits(p.nmax);
  if (tail) {
    // a block per 1024 entries if every candidate is evaluated (blocks without entries exit at once), then one block
    const StagedTailArgs ta{a.lpart, cap,     ls,   a.seeds, a.surv,  Nc,       cand,   p.D,     p.Pb(),
                            a.el,    a.eg,    a.lo, a.U,     a.flags, a.first1, a.list, a.count, a.rescue,
                            a.stage, p.floor};
    hipLaunchKernelGGL(staged_tail_kernel, dim3((unsigned)((Nc + cap + 1023) / 1024)), dim3(256), 0, s, ta);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(staged_shortlist_kernel, dim3(1), dim3(TAIL_THREADS), 0, s, ta);
  } else {
    hipLaunchKernelGGL(staged_merge_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, a.lpart, cap, ls,
                       a.surv, (const int32_t*)a.stage + HBX_ST_NSURV, (int32_t)Nc, a.el, a.eg, p.Pb(), a.stage, 0,
                       p.floor);
  }
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

// Stage 1 of the last single acquisition on this workspace (device read, synchronises): out[0] = 1 when lhi and
// Lmax came from the scoring kernel's epilogue (0: from staged_l_kernel, or the call did not stage), out[1] = the
// state words' Lmax, an order-preserving uint of the float.
int hbx_kde_acquire_stage1(const void* workspace, int64_t Nc, int64_t nmax, int64_t* out) {
  if (!workspace || !out || Nc < 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_acquire_stage1: bad arguments");
  const WsLayout w = ws_layout(Nc, nmax);
  uint32_t st[HBX_ST_WORDS];
  HBX_HIP(hipDeviceSynchronize());
  HBX_HIP(hipMemcpy(st, (const char*)workspace + w.stage, sizeof(st), hipMemcpyDeviceToHost));
  out[0] = st[HBX_ST_FLAG] == 1 && st[HBX_ST_LHI1] == 1 ? 1 : 0;
  out[1] = (int64_t)st[HBX_ST_LMAX];
  return HBX_OK;
}

}  // extern "C"
