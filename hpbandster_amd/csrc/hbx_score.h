// hbx_score.h -- launch-side scoring dispatch.  Users: hbx_score.hip (defines it; hbx_kde_logpdf),
// hbx_kde.hip (acq_score: the acquisitions' scoring launch; the workspace's split bound), hbx_staged.hip (stage 1's
// pair shape, the list launches' splits) and hbx_topk.hip (through acq_score).
#pragma once
#include "hbx_kde_impl.h"

#define OBS_SPLIT_MAX 16  // observation splits of one scoring launch at most (obs_splits)

struct ScoreFns {
  logpdf_fn main, rescue;
  int cands_per_block;
  int threads;
  logpdf_pair_fn pair;  // the same kernel over both KDEs in one grid (hmode 16x16 only), or nullptr
  logpdf_pair_fn rescue_pair;
  bool split_ok = false;  // the pair kernel takes observation splits and initialises a single acquisition's
                          // state (the 32x32-tile instances); a combine kernel may then do the rescue pass
  logpdf_pair_fn pair1 = nullptr;  // the coarse pair kernel with one column tile per wave (pair_shape)
  logpdf_list_fn list = nullptr;   // the coarse instance over an index list (the staged acquisition)
  logpdf_co_fn main_co = nullptr;  // the coarse instance over one KDE: launch_score runs it in main's place
};

// variant: a prepared KDE's code (KdeVariant, hbx_kde_impl.h)
// fast: the acquisition's instance where one exists (the 32x32 kernel without the one-hot lo steps,
// their bound added) -- its ln-pdf estimates are looser than 1e-5, so calls that report them do not use it
ScoreFns pick_logpdf(int dc_pad, int du_pad, int variant, bool fast);

// Observation splits of a pair launch with `tiles` candidate tiles per KDE over <= nmax observations
// (HBX_OBS_SPLIT=0: none; ws_sizing: the workspace's bound, no switch) ...
int obs_splits(unsigned tiles, int64_t nmax, bool ws_sizing);
// ... and of a list launch (the staged acquisition's bad-KDE launches)
int list_splits(int64_t nmax);

// The shape of a pair launch over Nc candidates: the kernel (f.pair, or f.pair1 -- one column tile per wave -- while
// the launch fits one round of the chip's block slots), its candidate tiles per KDE, its observation splits per
// KDE (split_nmax: the observation count they are sized for, 0: none).  kdes: how many KDEs' blocks share the
// slots -- 2 in the fused launch (2 tiles <= 512), 1 where the good KDE has them to itself (stage 1 of the staged
// acquisition: tiles <= 512, so between 131k and 262k candidates it runs another instance than the fused launch
// would; the sums do not depend on it).  pair1_ok: every KDE of the launch has the same pair1 instance.
// HBX_PAIR1=0: always f.pair; HBX_OBS_SPLIT=0: no splits (both read per call: tests switch them in-process).
// HBX_ROW_STAGE=0 (hbx_row_stage, read per call like them): the coarse instances read their candidate rows in
// place instead of staging them through LDS (KdePairArgs::row_stage; the sums do not depend on it).
struct PairShape {
  logpdf_pair_fn kernel;
  unsigned tiles;
  int nsplit;
};
PairShape pair_shape(const ScoreFns& f, bool pair1_ok, int kdes, int64_t Nc, int64_t split_nmax);
static inline int32_t hbx_row_stage() { return hbx_switch_on("HBX_ROW_STAGE") ? 1 : 0; }

// launch main + rescue scoring for one KDE
int launch_score(ScoreFns f, const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                 KdeEst* est, hipStream_t s);

// One KDE's side of an acquisition's scoring launch, what the launch is asked for, and what it did
struct ScoreSide {
  ScoreFns f;
  const void* params;
  const float* table;
  KdeEst* est;
};
struct ScoreRequest {
  const double* cand;
  int64_t Nc;
  int32_t D;
  hipEvent_t* ev;       // timing, or nullptr: [0] before, [1] after the good KDE's launches, [2] after the bad
                        // one's; a pair launch stamps [0] and [1] only ([1] after everything)
  int32_t* rescue_cnt;  // the workspace's marker counter
  KdePairArgs::AcqInitPtrs init;  // a single acquisition's state for the launch to initialise (U null: none)
  int64_t split_nmax;             // observations the splits are sized for (0: no splits)
  bool combine_rescues;           // the caller's combine kernel can do the rescue pass
  hipStream_t s;
};
struct ScoreResult {
  bool inited = false;         // the launch (or its rescue pass) initialises the state in rq.init
  bool rescue_inline = false;  // the rescue pass is left to the combine kernel
  int32_t nsplit[2] = {1, 1};  // observation splits of the good / bad KDE's estimates
};
// launch main + rescue scoring for both KDEs of an acquisition: one pair launch when both run the same hmode
// instance (the bad KDE -- normally the larger -- first; HBX_SCORE_PAIR=0: never), else two single launches
int launch_score2(const ScoreSide& good, const ScoreSide& bad, const ScoreRequest& rq, ScoreResult* out);
