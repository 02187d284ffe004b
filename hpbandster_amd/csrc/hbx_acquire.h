// hbx_acquire.h -- what the acquisitions of one KDE pair share on the launch side.  Users: hbx_kde.hip
// (defines it; the argmin: single, bound, batched), hbx_staged.hip (acq_score_staged), hbx_topk.hip (the top-k of
// one pool, which runs the same scoring and exact re-score around its own selection steps) and hbx_exact.hip
// (acq_exact, beside its kernels).
#pragma once
#include "hbx_score.h"

// A prepared (good, bad) KDE pair: what hbx_kde_pair_bind returns and every acquisition entry point takes
struct KdePairRef {
  int32_t D;
  const void* params_good;
  const float* table_good;
  const double* X_good;
  const int64_t* rows_good;
  int32_t variant_good;
  const void* params_bad;
  const float* table_bad;
  const double* X_bad;
  const int64_t* rows_bad;
  int32_t variant_bad, dc_pad, du_pad;
  int64_t nmax;
  ScoreFloor floor;  // the score floor of every acquisition on the handle (hbx_kde_pair_set_rules)
  const KdeParams* Pg() const { return (const KdeParams*)params_good; }
  const KdeParams* Pb() const { return (const KdeParams*)params_bad; }
};

// workspace layout (bytes), shared by the *_workspace_bytes helpers and the acquisitions; B = number
// of acquisitions (segments) of a batched call (1 for hbx_kde_acquire).  The single result record
// comes first so its offset does not depend on the sizes.
struct WsLayout {
  size_t res, U, count, flags, segcnt, segnear, best, key, first1, rescue, est_l, est_g, lo, list, near, exact_l,
      exact_g, part, total;
  // the staged single acquisition (hbx_staged.hip), appended: its state words (in the result slot's padding),
  // the seed list (list_cap entries), the survivor list (Nc), the list launches' split partials
  // ([OBS_SPLIT_MAX][list_cap] estimates), stage 1's block maxima (a float per 256 candidates: a block of either
  // coarse pair kernel covers 256 or 512)
  size_t stage, seeds, surv, lpart, bmax;
  int32_t list_cap;
};
#define STAGED_LIST_CAP 4096  // seeds at most, and listed candidates at most of a split list launch
WsLayout ws_layout(int64_t Nc, int64_t nmax, int64_t B = 1);

// the workspace's arrays as typed pointers
struct AcqWs {
  AcqResult* res;
  uint32_t* U;
  int32_t *count, *flags, *segcnt, *segnear;
  uint64_t *best, *key;
  int32_t *first1, *rescue;
  KdeEst *el, *eg;
  float* lo;
  int32_t *list, *near;
  double *exact_l, *exact_g, *part;
  uint32_t* stage;
  int32_t *seeds, *surv;
  KdeEst* lpart;
  float* bmax;
  int32_t list_cap;
  AcqWs(void* workspace, const WsLayout& w) {
    char* ws = (char*)workspace;
    res = (AcqResult*)(ws + w.res);
    U = (uint32_t*)(ws + w.U);
    count = (int32_t*)(ws + w.count);
    flags = (int32_t*)(ws + w.flags);
    segcnt = (int32_t*)(ws + w.segcnt);
    segnear = (int32_t*)(ws + w.segnear);
    best = (uint64_t*)(ws + w.best);
    key = (uint64_t*)(ws + w.key);
    first1 = (int32_t*)(ws + w.first1);
    rescue = (int32_t*)(ws + w.rescue);
    el = (KdeEst*)(ws + w.est_l);
    eg = (KdeEst*)(ws + w.est_g);
    lo = (float*)(ws + w.lo);
    list = (int32_t*)(ws + w.list);
    near = (int32_t*)(ws + w.near);
    exact_l = (double*)(ws + w.exact_l);
    exact_g = (double*)(ws + w.exact_g);
    part = (double*)(ws + w.part);
    stage = (uint32_t*)(ws + w.stage);
    seeds = (int32_t*)(ws + w.seeds);
    surv = (int32_t*)(ws + w.surv);
    lpart = (KdeEst*)(ws + w.lpart);
    bmax = (float*)(ws + w.bmax);
    list_cap = w.list_cap;
  }
  // a single acquisition's state, for the launch that initialises it
  KdePairArgs::AcqInitPtrs init() const { return {U, count, flags, first1, res}; }
};

// The steps every acquisition runs, in this order around its own selection steps.
// (1) the pointer and range checks, then both KDEs' scoring instances (fast: no ln-pdf estimates reported)
struct AcqPlan {
  ScoreFns fg, fb;
  bool exact_only;  // a KDE outside every fp32 scoring bucket: no scoring launch, every candidate re-scored
};
const KdePairRef* acq_pair(const char* who, const void* pair);  // an entry point's handle; NULL: HBX_ERR_ARG is set
int acq_check(const char* who, const KdePairRef& p, const double* cand, int64_t Nc, const void* workspace);
int acq_plan(const KdePairRef& p, bool fast, AcqPlan* plan);
// (2) the scoring launch (first: it touches none of the per-acquisition state, so the GPU starts on it while
// the host enqueues the rest; launch_score2, hbx_score.h, which also documents rq and out), then the state's
// initialisation where the launch did not do it (batch_B > 0: the B segments' state instead, rq.init empty), then
// the launch's observation splits merged.  The estimates land in a.el / a.eg.
int acq_score(const AcqPlan& plan, const KdePairRef& p, const AcqWs& a, const ScoreRequest& rq, int64_t batch_B,
              ScoreResult* out);
// (2') instead of (2) for a single acquisition without ln-pdf outputs whose KDEs both run the coarse 32x32
// instance: the staged scoring (hbx_staged.hip) -- l for every candidate, g only where l alone does not rule the
// candidate out; without the short tail (below) the others' a.eg holds the marker HBX_EST_NOT_EVAL, which the
// combine kernel reads as an l-only interval, and the rescue of marked g estimates is left to that kernel (its
// <_, true> instance).
// events: [0] at the first scoring launch's start, [1] and [2] after the last one.
// Whether a call stages: HBX_STAGED (hbx_staged_mode, hbx_common.h) and, by size, HBX_STAGED_MIN_PAIRS.
#ifndef HBX_STAGED_MIN_PAIRS
#define HBX_STAGED_MIN_PAIRS 1e9  // candidates x observations from which an acquisition stages when HBX_STAGED is unset
#endif
// The top-k of one pool (hbx_topk.hip "Staged scoring") stages from a higher size: its selection costs eight more
// launches than the argmin's, so where l prunes everything it breaks even at 9e8 pairs and gains 1.9-2.4x at
// 4.9e9, and where nothing is pruned it pays 16-17 % at 1e10 (measured, profiles/staged_topk/README.md).
#ifndef HBX_STAGED_TOPK_MIN_PAIRS
#define HBX_STAGED_TOPK_MIN_PAIRS 4e9
#endif
// tail (HBX_STAGED_TAIL, hbx_common.h): the short tail -- the call also leaves every candidate's a.lo, a.U,
// a.first1, the overflow flag, the shortlist a.list / a.count and the marker count zeroed, the unevaluated
// candidates' a.eg unwritten: no combine and no shortlist launch behind it.
bool acq_staged_supported(const AcqPlan& plan);
int acq_score_staged(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                     hipEvent_t* ev, hipStream_t s, bool tail);
// acq_score_staged's launches step by step, shared with the staged top-k (hbx_topk.hip), which puts its own
// thresholds between them:
//   staged_score_l          stage 1: the good KDE's pair kernel, then staged_l_kernel (lhi into a.lo, Lmax into the
//                           state words).  lkey non-null: also every candidate's ordered key of -llo (+inf: no finite
//                           llo) and the hist_words words at hist zeroed.  lhi_blocks non-null (the argmin): where
//                           the launch runs unsplit and HBX_STAGE1_LHI is not 0, the pair kernel's epilogue leaves
//                           lhi and one maximum per block in a.bmax instead, staged_l_kernel is not launched, and
//                           *lhi_blocks is the block count (else 0) -- to be handed to staged_score_seeds, whose
//                           seed kernel then reduces the maxima itself
//   staged_score_seeds      stages 2 and 3: the seed list against the threshold in the state words' Lmax, the bad
//                           KDE's list launch over it, its partials merged and scattered (update_u: U_seed lowered
//                           to the seeds' smallest upper score bound)
//   staged_score_survivors  stage 4: the survivor list against the state words' U_seed (lonly: a.lo becomes the
//                           l-only lower score bound, lhi > 700 raises the overflow flag) and the list launch over it;
//                           its partials, where it ran split, are left to the caller
int staged_score_l(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                   hipEvent_t* ev, hipStream_t s, uint32_t* lkey, uint32_t* hist, int32_t hist_words,
                   unsigned* lhi_blocks = nullptr);
int staged_score_seeds(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                       hipStream_t s, bool mark_rest, bool update_u, unsigned lhi_blocks = 0);
int staged_score_survivors(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a,
                           hipStream_t s, bool lonly);
// exact-only acquisitions instead of a combine / bounds pass: every candidate joins the re-score
int acq_exact_only_init(int64_t Nc, uint32_t seg, const AcqWs& a, hipStream_t s);
// (3) the exact fp64 re-score of the shortlist a.list / a.count (scan, a single acquisition of at most
// EXACT_SCAN_MAX candidates: the blocks shortlist for themselves), then -- combine -- its unit sums into
// a.exact_l / a.exact_g; wide: behind the staged acquisition's short tail (short shortlists: the re-score's wide
// blocks, hbx_exact.hip; never together with scan)
#define EXACT_SCAN_MAX 1024
int acq_exact(const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a, bool scan, bool combine,
              hipStream_t s, bool wide = false);
