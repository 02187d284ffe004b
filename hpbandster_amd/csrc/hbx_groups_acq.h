// hbx_groups_acq.h -- what the grouped acquisitions' files share beyond hbx_groups_impl.h: the argument block of one
// call, the empty record and the frame of the select kernels.  hbx_groups.hip (the screens, the floored select, the top-k, every host check) and
// hbx_groups_lr.hip (the log-ratio select) include it; the definitions stood in hbx_groups.hip before the second file.
#pragma once
#include "hbx_groups_impl.h"

// The acquisition's reading of grp_classify's bits (hbx_groups_impl.h), stated here and nowhere else: a group is
// exact-only -- re-scored whole, HBX_ACQ_OVERFLOW -- when either of its KDEs cannot be screened (GRP_EXACT(kd)); a
// negative match factor (h > 1, GRP_NEG(kd)) is screened like any other KDE, as a signed sum.
#define GRP_EXACT_ONLY GRP_EXACT_ANY
#define GRP_NO_SCREEN (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY)

#define GRP_WS_HEAD 256  // the workspace's head: the counters; the screen slots follow

struct GrpArgs {
  GrpModel M;
  const double* cand;
  int64_t S, C;      // requests per group (1: hbx_kde_acquire_groups), candidates per request
  int64_t P;         // S * C: the group's flattened pool, what the screen sees
  int32_t tiles;     // ceil(P / 64)
  int32_t slabs;     // tile screen: blocks per group, one tile per wave
  GScreen* scr;
  AcqResult* res;
  ScoreFloor F;      // the call's score floor (hbx_rules.pdf_floor), read by the kernels' <.., DEFF = false> instances
  // the request mask (hbx_kde_acquire_groups_batch_m), read by the kernels' <.., MASK = true> instances alone:
  const uint8_t* want;         // u8[B][S], request (b, s) is answered when its byte is not 0; NULL: every request
  unsigned long long* stats;   // the workspace head's counters (hbx_kde_groups_request_stats)
};

__device__ __forceinline__ AcqResult grp_empty_record(int32_t flags) {
  AcqResult r;
  r.index = -1;
  r.score = r.pdf_l = r.pdf_g = NAN;
  r.rel = 0.f;
  r.flags = flags;
  r.shortlist = 0;
  r.near = 0;
  return r;
}

// ---- the frame of the select kernels (groups_select_kernel, groups_select_lr_kernel) --------------------------
// One block per request q of group b.  Each kernel keeps its pass 1, the body of its pass 2 and its counters.

// The prologue (whole block, ends with a barrier: what thread 0 initialised before the call is visible after it):
// wave 0 classifies the group, *st = grp_classify's bits.  Returns true when the request's record is written and the
// block returns: the skipped record, carrying the group's bits as the dense call sets them, where `want` (nullable)
// leaves q out; the empty record where the group has no model or is unsupported.  `answered`: flags every answered
// record carries; `count`: whether answered requests are counted (skipped ones always are).
__device__ __forceinline__ bool grp_select_prologue(const GrpArgs& A, int64_t q, int64_t b, const uint8_t* want,
                                                    bool count, int32_t answered, int32_t* s_st, int* st) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    int dc, du;
    const int st0 = grp_classify(A.M, b, &dc, &du);
    if (tid == 0) *s_st = st0;
  }
  __syncthreads();
  *st = *s_st;
  const int32_t gbits = (*st & GRP_NO_MODEL) ? HBX_ACQ_NO_MODEL : (*st & GRP_UNSUPPORTED) ? HBX_ACQ_UNSUPPORTED : 0;
  if (want && want[q] == 0) {  // (uniform)
    if (tid == 0) {
      A.res[q] = grp_empty_record(HBX_ACQ_SKIPPED | gbits);
      atomicAdd(A.stats + 1, 1ull);
    }
    return true;
  }
  if (gbits) {
    if (tid == 0) {
      A.res[q] = grp_empty_record(answered | gbits);
      if (count) atomicAdd(A.stats + 0, 1ull);
    }
    return true;
  }
  return false;
}

// The group's observations and the row positions of its good and bad KDE in them; threads 0 and 1 fill vw[2].
// (Out-parameters: returned as a struct, the same three pointers cost groups_select_lr_kernel 8 VGPRs and a wave per
// SIMD, 133 against 125.)
__device__ __forceinline__ void grp_rows(const GrpModel& M, int64_t b, GrpView* vw, const double** Xs,
                                         const int64_t** rows_g, const int64_t** rows_b) {
  const int64_t s0 = M.seg_off[b], n = M.seg_off[b + 1] - s0;
  *Xs = M.X + s0 * M.D;
  *rows_g = M.order + s0;
  *rows_b = M.order + s0 + (n - M.n_bad[b]);
  if (threadIdx.x < 2) vw[threadIdx.x] = grp_view(M, b, threadIdx.x);
}

// The tail (whole block): thread 0 hands its winner over -- best score, index bidx (-1: none), the exact pdfs bl, bg
// --, the block counts the near set, every re-scored candidate (GS_DONE, its exact score in its slot) the winner cannot
// be told apart from by the bounds: near(s, rel, best, rel_best); thread 0 writes the record A.res[q].  `more_near`: candidates
// that tie with the winner without having been re-scored (thread 0's value).
template <class Near>
__device__ __forceinline__ void grp_select_tail(const GrpArgs& A, int64_t q, const GScreen* scr, int64_t C, double best,
                                                int64_t bidx, double bl, double bg, int32_t nshort, int32_t flags,
                                                int32_t more_near, Near near) {
  __shared__ double s_best, s_rb;
  __shared__ int64_t s_bidx;
  __shared__ int32_t s_near;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_best = best;
    s_bidx = bidx;
    s_rb = bidx >= 0 ? (double)scr[bidx].rel : 0.0;
    s_near = 0;
  }
  __threadfence_block();
  __syncthreads();  // (also: thread 0's stores to scr are visible to the block)
  const double sb = s_best, rb = s_rb;
  const int64_t wi = s_bidx;
  if (wi >= 0) {
    int cnt = 0;
    for (int64_t i = tid; i < C; i += GRP_SEL_THREADS) {
      const GScreen g = scr[i];
      if (!(g.fl & GS_DONE)) continue;
      if (i == wi || near(g.score, (double)g.rel, sb, rb)) ++cnt;
    }
    if (cnt) atomicAdd(&s_near, cnt);
  }
  __syncthreads();
  if (tid == 0) {
    AcqResult r = grp_empty_record(flags);
    r.shortlist = nshort;
    r.near = s_near + more_near;
    r.rel = (float)rb;
    if (r.near > 1) r.flags |= HBX_ACQ_NEAR_TIE;
    if (wi >= 0) {
      r.index = wi;
      r.score = sb;
      r.pdf_l = bl;
      r.pdf_g = bg;
    }
    A.res[q] = r;
  }
}

// hbx_groups_lr.hip: the log-ratio select over the slots that the screens' <.., LR = true> instances wrote, one block
// per request; `masked`: A.want may leave requests out (groups_select_lr_kernel<true>)
void grp_launch_select_lr(const GrpArgs& A, bool masked, hipStream_t s);
