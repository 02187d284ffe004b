// hbx_score.h -- launch-side scoring dispatch.  Users: hbx_score.hip (defines it; hbx_kde_logpdf),
// hbx_kde.hip (the acquisitions' scoring launch, the workspace's split bound) and hbx_topk.hip (the top-k
// acquisition's scoring launch).
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
  logpdf_pair_fn pair1 = nullptr;  // the coarse pair kernel with one column tile per wave (launch_score2)
  logpdf_list_fn list = nullptr;   // the coarse instance over an index list (the staged acquisition)
};

// variant code of a prepared KDE (hbx_kde_prepare info[0]): bit 0 = signed sums, bits 1-3 = kc,
// bit 4 = hmode (whole exponent on the f16 matrix cores), bit 6 = its 32x32-tile kernel (h32 table)
// fast: the acquisition's instance where one exists (the 32x32 kernel without the one-hot lo steps,
// their bound added) -- its ln-pdf estimates are looser than 1e-5, so calls that report them do not use it
ScoreFns pick_logpdf(int dc_pad, int du_pad, int variant, bool fast = false);

// Observation splits of a pair launch with `tiles` candidate tiles per KDE over <= nmax observations
// (HBX_OBS_SPLIT=0: none; ws_sizing: the workspace's bound, no switch)
int obs_splits(unsigned tiles, int64_t nmax, bool ws_sizing = false);

// launch main + rescue scoring for one KDE
int launch_score(ScoreFns f, const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                 KdeEst* est, hipStream_t s);

// launch main + rescue scoring for both KDEs of an acquisition: one pair launch when both run the
// same hmode instance (KDE 1 -- the bad one, normally the larger -- first), else two single launches.
// Events (optional): [0] before, [1] after KDE 0's launches, [2] after KDE 1's; a pair launch
// records [0] and [1] only ([1] after everything).
int launch_score2(ScoreFns f0, const void* params0, const float* table0, KdeEst* est0, ScoreFns f1,
                  const void* params1, const float* table1, KdeEst* est1, const double* cand, int64_t Nc, int32_t D,
                  hipEvent_t* ev, int32_t* rescue_cnt, hipStream_t s, KdePairArgs::AcqInitPtrs init = {},
                  bool* inited = nullptr, int64_t nmax = 0, int32_t* nsplit_out = nullptr,
                  bool* rescue_inline = nullptr);
