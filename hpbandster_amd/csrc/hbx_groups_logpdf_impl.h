// hbx_groups_logpdf_impl.h -- what the grouped ln-pdf's two files share (hbx_groups_logpdf.hip: the status kernel, the
// fp32, fp64 and exact passes and the entry point; hbx_groups_logpdf_signed.hip: the signed log-space pass): the
// launch arguments, the workspace header and the status bits of one KDE.
#pragma once
#include "hbx_groups_impl.h"

#define GLP_HEAD 256  // workspace header: the four counters (u64) in its first 32 bytes
#define GLP_BAD (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED)
#define GLP_EXACT_BIT(kd) ((kd) ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L)     // every value through the exact pdf
#define GLP_SIGNED_BIT(kd) ((kd) ? HBX_GRP_SIGNED_G : HBX_GRP_SIGNED_L)  // the signed pass, its list through the exact pdf

struct GlpArgs {
  GrpModel M;
  const double* cand;
  int64_t C;
  int32_t tiles;     // ceil(C / 64)
  int32_t kd0;       // first KDE of the launch's grid.y (0: good / ln_l, 1: bad / ln_g)
  int32_t fp64_only;
  int32_t signed_route;  // HBX_LOGPDF_SIGNED: KDEs with a negative match factor take the signed pass
  double rtol;
  double* out[2];    // ln_l, ln_g (nullable)
  int32_t* status;
  unsigned long long* stat;  // the header's counters
  int32_t* cnt;              // [B][2] listed candidates per (group, KDE)
  int32_t* list;             // [B][2][C]
};

// The lanes of one wave that hold a candidate without a written value (`listed`) append their indices i to the
// (group, KDE)'s list segment: one atomic per tile; the segment holds C entries and a candidate is listed once.
__device__ __forceinline__ void glp_list_append(const GlpArgs& A, int64_t b, int kd, bool listed, int64_t i, int lane) {
  const uint64_t bal = __ballot(listed);
  if (!bal) return;
  const int first = __ffsll((long long)bal) - 1;
  int32_t base = 0;
  if (lane == first) base = atomicAdd(&A.cnt[b * 2 + kd], __popcll(bal));
  base = __shfl(base, first);
  if (listed) A.list[(b * 2 + kd) * A.C + base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)i;
}

// the signed pass's launch (hbx_groups_logpdf_signed.hip): the bucket's instance, fp64 exponentials for rtol < 1e-5
int glp_signed_launch(const GlpArgs& A, dim3 grid, hipStream_t s);
