// hbx_prep.h -- model preparation's interface inside the library.  Users: hbx_prep.hip (the preparation
// kernels, prep_args / prep_launch, hbx_kde_prepare), hbx_refit.hip (the one-call refit fills a PrepSet and
// launches it) and hbx_score.hip (bucket_dims: the scoring instance of a bucket).
#pragma once
#include "hbx_kde_impl.h"

__host__ __device__ static void bucket_dims(int dc, int du, int* dc_pad, int* du_pad) {
  const int dcb[] = {0, 4, 8, 16, 24, 32, 64};
  const int dub[] = {0, 4, 8, 16, 32};
  *dc_pad = -1;
  *du_pad = -1;
  for (int b : dcb)
    if (dc <= b) { *dc_pad = b; break; }
  for (int b : dub)
    if (du <= b) { *du_pad = b; break; }
}

// Model preparation runs on the device from (data rows, bandwidths, level counts), so a refit needs
// no host round trip until its single read-back (hbx_kde_refit).  One or two KDEs per launch
// (PrepSet): block / block range k belongs to KDE k.
struct PrepArgs {
  const double* X;      // device f64[*][D]
  const int64_t* rows;  // device i64[n]
  const double* bw;     // device f64[D]
  const int32_t* nlev;  // device i32[D]
  KdeParams* P;
  int32_t* info;        // device i32[8]
  int32_t n, D;
  int32_t hm_allowed;   // HBX_HMODE not 0
  int32_t h32_allowed;  // HBX_H32 not 0
  int32_t co_allowed;   // HBX_COARSE not 0: the coarse h32 table beside the precise one
  int32_t nblk_table;   // blocks of this KDE in the table launches
  uint32_t vt[HBX_MAX_D / 32];  // bit d: dim d categorical ('u')
};
// The refit's output block published to device-mapped host memory (hbx_kde_refit_sync), every 32-bit word of it
// as one flagged 8-byte word (seq << 32 | word): the split's rows (n words: indices < 2^31), each KDE's
// bandwidths (2 D words: the doubles' low then high halves) and level counts (D words) by the parameter
// launch, then the two info records (16 words, `ll`) by the finishing blocks.  The host accepts a word only when
// it carries the call's sequence number, so it needs no ordering between the launches' stores and the host
// (dst == nullptr: nothing published)
struct PrepPub {
  uint64_t* dst;        // mapped flagged words: order [0, n), bw KDE k [n + 2 D k, + 2 D), nlev KDE k [n + 4 D + D k, + D)
  const uint32_t* src;  // the device output block
  uint64_t* ll;         // the two info records as 16 flagged words
  int32_t seq;
  int32_t n;            // rows of the split
  int32_t bw_off[2], nl_off[2], info_off[2];  // word offsets of KDE k's pieces in src
  int32_t D;
};
struct PrepSet {
  PrepArgs k[2];
  int32_t nk;
  PrepPub pub;
};

__host__ __device__ __forceinline__ ColStats* col_stats(KdeParams* P) { return (ColStats*)((char*)P + HBX_COLSTATS_OFF); }

// host: fill a PrepArgs (vartype from host memory), checking the table capacity
int prep_args(PrepArgs* A, const double* X, int32_t D, const int64_t* rows, int32_t n, const int32_t* vartype,
              const double* bw, const int32_t* nlev, void* params, int32_t* info, int64_t table_floats_);

// enqueue the preparation of ps.nk KDEs (no host synchronisation).  colstats_done: the fit wrote the column
// statistics already (refit_fit_colstats)
int prep_launch(PrepSet& ps, float* table0, float* table1, hipStream_t s, bool colstats_done = false);
