// hbx_groups_acq.h -- what the grouped acquisitions' files share beyond hbx_groups_impl.h: the argument block of one
// call and the empty record.  hbx_groups.hip (the screens, the floored select, the top-k, every host check) and
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

// hbx_groups_lr.hip: the log-ratio select over the slots that the screens' <.., LR = true> instances wrote, one block
// per request; `masked`: A.want may leave requests out (groups_select_lr_kernel<true>)
void grp_launch_select_lr(const GrpArgs& A, bool masked, hipStream_t s);
