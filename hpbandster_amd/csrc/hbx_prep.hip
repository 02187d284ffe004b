// hbx_prep.hip -- model preparation on MI355X (gfx950): a KDE's parameter block and chunked observation table
// built on the device from (data rows, bandwidths, level counts).
//
//   kde_colstats     per (KDE, dim): the column mean / the largest categorical code
//   kde_params       the parameter block (KdeParams), the one-hot layout, the scoring mode
//   kde_table        the observation table in the layout of that mode (hbx_kde_impl.h); a KDE's last block
//                    rebuilds it in the f32 layout when C_j left the f16 range and writes the info record
//   kde_prep_finish  the info record as a launch of its own (sets with an exact-only KDE)
// hbx_kde_prepare prepares one KDE from host inputs; the one-call refit (hbx_refit.hip) both KDEs of a budget.
#include <math.h>
#include <string.h>

#include "hbx_prep.h"
#include "hbx_sort.h"  // lane_xor_u32

__host__ __device__ static int table_stride(int dc_pad, int du_pad) { return chunk_floats(dc_pad, du_pad); }
static int64_t n_chunks(int64_t n) { return (n + OBS_CHUNK - 1) / OBS_CHUNK; }
__device__ __forceinline__ int64_t n_chunks_dev(int64_t n) { return (n + OBS_CHUNK - 1) / OBS_CHUNK; }
// capacity of a table: the largest layout hbx_kde_prepare may choose for this bucket (exact-only KDEs,
// outside every bucket, keep no table: one float)
static int64_t table_floats(int64_t n, int dc_pad, int du_pad) {
  if (dc_pad < 0 || du_pad < 0) return 1;
  int a = chunk_floats(dc_pad, du_pad, 0, 0), b = chunk_floats(dc_pad, du_pad, OH_MAX_KC, 1);
  const int c = h_chunk_floats(dc_pad, OH_MAX_KC, 1), d = h32_chunk_floats(nsc_of(dc_pad), OH_MAX_KC, 1);
  a = a > b ? a : b;
  a = a > d ? a : d;
  // + the coarse h32 table (hbx_kde_impl.h), after the main one
  const int e = h32c_chunk_floats(nsc_of(dc_pad), 2);
  return n_chunks(n) * (int64_t)((a > c ? a : c) + e);
}

// The split's rows (KDE 0) and KDE k's bandwidths and level counts -- written by the launches before the
// parameter launch -- published by the parameter launch's block k (thread t of nt) as flagged words: the rows
// of a 400-observation refit are ~2 stores per thread, not 14 dependent load/store pairs of one wave
__device__ __forceinline__ void prep_publish_rows(const PrepPub& q, int k, int t, int nt) {
  const uint64_t tag = (uint64_t)(uint32_t)q.seq << 32;
  auto put = [&](int64_t i, uint32_t w) {
    __hip_atomic_store(q.dst + i, tag | w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  if (k == 0) {
    const int64_t* order = (const int64_t*)q.src;  // (the order sits at word 0 of the block)
    for (int i = t; i < q.n; i += nt) put(i, (uint32_t)order[i]);
  }
  const int64_t bw0 = (int64_t)q.n + 2 * (int64_t)q.D * k, nl0 = (int64_t)q.n + 4 * (int64_t)q.D + (int64_t)q.D * k;
  for (int i = t; i < 2 * q.D; i += nt) put(bw0 + i, q.src[q.bw_off[k] + i]);
  for (int i = t; i < q.D; i += nt) put(nl0 + i, q.src[q.nl_off[k] + i]);
}
// KDE k's info record (from registers) as flagged 8-byte words: (prep_publish_info below reads it back)
__device__ __forceinline__ void prep_publish_vals(const PrepPub& q, const int32_t (&vals)[8], int k) {
  for (int i = 0; i < 8; ++i)
    __hip_atomic_store(q.ll + 8 * k + i, ((uint64_t)(uint32_t)q.seq << 32) | (uint32_t)vals[i], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// KDE k's info record (thread 0's own stores of prep_finish_one, read back by it) as flagged 8-byte words:
// each carries the call's sequence number beside its value, so the host knows every word from the word itself
// and no store has to wait for the others' acknowledgement (a completion word after an acknowledged record
// cost ~12k cycles of round trip to host memory).  The host (hbx_kde_refit_sync) reads only tagged words, each
// accepted on its own tag: nothing guarantees it that the stream has completed.
__device__ __forceinline__ void prep_publish_info(const PrepPub& q, const PrepArgs& A, int k) {
  for (int i = 0; i < 8; ++i)
    __hip_atomic_store(q.ll + 8 * k + i, ((uint64_t)(uint32_t)q.seq << 32) | (uint32_t)A.info[i], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ bool prep_cat(const PrepArgs& A, int d) { return (A.vt[d >> 5] >> (d & 31)) & 1u; }


// Column statistics of every (KDE, dim), one workgroup each (blocks [k*D, (k+1)*D) belong to KDE k):
// the mean of a continuous column (the centre of the scaled coordinates: any finite centre is correct
// -- table and candidates use the same one -- it only keeps the fp32 expansion well conditioned, so the
// summation order is free) and the largest code of a categorical column.
__global__ __launch_bounds__(256) void kde_colstats_kernel(PrepSet ps) {
  const PrepArgs& A = (int)blockIdx.x >= ps.k[0].D ? ps.k[1] : ps.k[0];
  const int d = blockIdx.x % ps.k[0].D;
  const int n = A.n, D = A.D;
  ColStats* cs = col_stats(A.P);
  __shared__ double red[4];
  __shared__ int mred[4];
  if (!prep_cat(A, d)) {
    double acc = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) acc += A.X[A.rows[j] * (int64_t)D + d];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) cs->mean[d] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n;
  } else {
    int m = -1;
    for (int j = threadIdx.x; j < n; j += 256) {
      const double v = A.X[A.rows[j] * (int64_t)D + d];
      m = max(m, (!(v >= 0.0 && v < 1024.0) || v != floor(v)) ? 100000 : (int)v);
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) mred[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int mm = max(max(mred[0], mred[1]), max(mred[2], mred[3]));
      cs->maxcode[d] = mm >= 100000 ? -1 : mm;
    }
  }
}

// the table launch's block counter of a KDE (in its parameter buffer's staging area, after the info
// record; zeroed by kde_params_kernel)
__device__ __forceinline__ int32_t* prep_counter(KdeParams* P) {
  return (int32_t*)((char*)P + HBX_PARAM_STAGE + 8 * HBX_MAX_D + 4 * HBX_MAX_D + 32);
}

// PREP_STAMPS (diagnostic builds only): s_memtime at the phase boundaries of the parameter build (block 0) and of
// the table launch (block 1's and the finishing block's thread 0) into a buffer of their own, read back by
// hbx_debug_prep_stamps; no stamp executes in the product build
#ifdef PREP_STAMPS
__device__ unsigned long long prep_stamps[32];
#define PSTAMP(i) \
  if (threadIdx.x == 0) prep_stamps[i] = __builtin_amdgcn_s_memtime()
#else
#define PSTAMP(i)
#endif

// LDS of the parameter build
struct ParamsScratch {
  double t0[HBX_MAX_D], t1[HBX_MAX_D], h[HBX_MAX_D], mean[HBX_MAX_D];
  int32_t c[HBX_MAX_D], maxc[HBX_MAX_D], cm[HBX_MAX_D], cd[HBX_MAX_D];
  int32_t ix[HBX_MAX_D];   // index of dim d within its class (continuous slot k, categorical slot u, constant dim)
  uint8_t kind[HBX_MAX_D]; // 0 continuous, 1 active categorical, 2 constant (one level; h = 0, or h > 0 and finite:
                           // the KDE is then exact-only), 3 unsupported
  int32_t ohs[HBX_MAX_D];  // first one-hot position of each active categorical dim's block
  int32_t du, dcp, dup, exo, neg, dc_tot, du_tot, dc, nconst, kc, tot;
};

// The parameter block P of one KDE (the whole workgroup calls it; P in global memory or in LDS): the per-dim
// transcendentals and fields in parallel (each dim's slot within its class from one wave's ballots), the
// sums by thread 0 in dim order, the one-hot layout and the kernel mode.
__device__ __forceinline__ void kde_params_body(const PrepArgs& A, KdeParams* P, const ColStats* cs, ParamsScratch& S) {
  const int D = A.D, n = A.n;
  const int tid = threadIdx.x;
  uint32_t* pz = (uint32_t*)P;
  for (int i = tid; i < (int)(sizeof(KdeParams) / 4); i += blockDim.x) pz[i] = 0u;
  if (tid == 0) S.neg = 0;
  // per dim: continuous -> ln h and the scale; categorical -> log2 of the match / mismatch factors, and its class
  const double LOG2E = 1.4426950408889634;
  if (blockIdx.x == 0) PSTAMP(0);
  for (int d = tid; d < D; d += blockDim.x) {
    const double h = A.bw[d];
    const int c = A.nlev[d];
    S.h[d] = h;
    S.c[d] = c;
    S.mean[d] = cs->mean[d];
    S.maxc[d] = cs->maxcode[d];
    if (!prep_cat(A, d)) {
      S.kind[d] = 0;
      S.t0[d] = (h > 0.0) ? log(h) : 0.0;
      S.t1[d] = (h > 0.0) ? sqrt(LOG2E / 2.0) / h : 0.0;
    } else {
      // single observed level: match -> 1, mismatch -> 0/0 = NaN (a constant dim).  The same level count under a
      // finite h > 0 (a fitted 0 clipped to hbx_rules.min_bandwidth, or an explicit bandwidth): match -> 1 - h,
      // mismatch -> h / 0 = +inf in the reference's arithmetic, so the pdf is finite, +inf or NaN (an inf beside
      // an underflowed 0 in the dim-ordered product) -- also a constant dim, and the KDE exact-only (below): the
      // fp64 evaluation decides every candidate.  c < 2 otherwise, h <= 0 or NaN (c == -1: codes not integers in
      // [0, 1024)): not modelled
      S.kind[d] = (c == 1 && (h == 0.0 || (h > 0.0 && h < INFINITY))) ? 2 : ((c < 2 || !(h > 0.0) || h != h) ? 3 : 1);
      const double a = 1.0 - h, b = h / (double)(c - 1);
      S.t0[d] = log2(b);
      S.t1[d] = (a == 0.0) ? -INFINITY : log2(fabs(a));
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) PSTAMP(1);
  if (tid < 64) {  // each dim's slot within its class: ballots over 64-dim groups, in dim order
    const uint64_t below = (1ull << tid) - 1ull;
    int bc = 0, bu = 0, bk = 0, nu = 0;
    for (int g = 0; g < D; g += 64) {
      const int d = g + tid;
      const int kd = d < D ? S.kind[d] : -1;
      const uint64_t mc = __ballot(kd == 0), mu = __ballot(kd == 1), mk = __ballot(kd == 2), ma = __ballot(kd >= 1);
      if (d < D) S.ix[d] = kd == 0 ? bc + __popcll(mc & below) : kd == 1 ? bu + __popcll(mu & below)
                                                                         : bk + __popcll(mk & below);
      bc += __popcll(mc);
      bu += __popcll(mu);
      bk += __popcll(mk);
      nu += __popcll(ma);
    }
    if (tid == 0) {
      S.dc_tot = bc;  // every continuous dim has a slot
      S.du_tot = nu;  // every categorical dim, active or not
      S.du = bu;
      S.nconst = bk;
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += blockDim.x) {
    const double h = S.h[d];
    const int kd = S.kind[d], ix = S.ix[d];
    P->vartype[d] = kd != 0 ? 1 : 0;
    P->nlev[d] = S.c[d];
    P->bw[d] = h;
    if (kd == 0) {
      P->cont_dim[ix] = d;
      const double m = S.mean[d];
      P->center[ix] = (m == m && m - m == 0.0) ? m : 0.0;
      if (!(h > 0.0)) {
        P->nan_all = 1;  // exp(-0/0) * ... / 0 -> NaN for every candidate
        P->cont_scale[ix] = 0.0;
      } else {
        P->cont_scale[ix] = S.t1[d];
      }
    } else if (kd == 2) {
      P->const_dim[ix] = d;
    } else if (kd == 3) {
      P->unsupported = 1;
    } else {
      const double a = 1.0 - h;
      P->cat_dim[ix] = d;
      P->cat_maxcode[ix] = S.maxc[d];
      S.cm[ix] = S.maxc[d];
      S.cd[ix] = d;
      P->cat_delta[ix] = (a == 0.0) ? -1e30f : (float)(S.t1[d] - S.t0[d]);
      P->cat_negf[ix] = (a < 0.0) ? 1.f : 0.f;
      if (ix < HBX_LO_TERMS) {  // (the one-hot table's f16 split of the delta, below)
        const float dl = fminf(fmaxf(P->cat_delta[ix], -60000.f), 60000.f);
        P->lo_term[ix] = fabsf(dl) < 60000.f ? fabsf(dl - (float)(_Float16)dl) : 0.f;
      }
      if (a < 0.0) {
        P->has_neg = 1;
        S.neg = 1;
      }
    }
  }
  if (tid == 0) {  // the sums in dim order (np.prod(bw[iscontinuous]) sequential: the reference's order)
    double sum_ln_h = 0.0, m0 = 0.0, lb_sum = 0.0, prod_bw_c = 1.0;
    float sad = 0.f;
    bool one_pos = false;  // a single-level categorical dim with h > 0
    // branch-free (a factor 1 or a term +0.0 where a dim does not count: exact), so the loads of several dims
    // are in flight at once
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      const int kd = S.kind[d];
      const double h = S.h[d], lb = S.t0[d], la = S.t1[d];
      prod_bw_c *= (kd == 0) ? h : 1.0;
      sum_ln_h += (kd == 0 && h > 0.0) ? lb : 0.0;
      m0 += (kd == 1) ? ((la > lb) ? la : lb) : 0.0;
      lb_sum += (kd == 1) ? lb : 0.0;
      sad += (kd == 1 && 1.0 - h != 0.0) ? fabsf((float)(la - lb)) : 0.f;
      one_pos = one_pos || (kd == 2 && h > 0.0);
    }
    int dcp, dup;
    bucket_dims(S.dc_tot, S.du_tot, &dcp, &dup);
    P->n = n;
    P->D = D;
    P->dc_pad = dcp;
    P->du_pad = dup;
    // exact-only: outside every bucket (the host knows: no table launch), or a single-level dim with h > 0 (the
    // table launch runs: the f32 layout, which no acquisition reads)
    const int exo = (dcp < 0 || dup < 0 || one_pos) ? 1 : 0;
    P->exact_only = exo;
    P->stride = (dcp < 0 || dup < 0) ? 0 : table_stride(dcp, dup);
    const int dc = S.dc_tot;
    P->dc = dc;
    P->du = S.du;
    S.dcp = dcp;
    S.dup = dup;
    S.exo = exo;
    P->nconst = S.nconst;
    P->m0_log2 = m0;
    P->lb_sum = lb_sum;
    P->prod_bw_c = prod_bw_c;
    P->sum_abs_delta = sad;
    const double log_norm = -log((double)n) - sum_ln_h - 0.5 * (double)dc * log(2.0 * M_PI) + m0 * M_LN2;
    P->log_norm = log_norm;
    P->lnpdf_guard = log_norm + log((double)(n > 1 ? n : 1)) < 600.0 ? 1 : 0;
    P->X = A.X;
    P->rows = A.rows;
  }
  __syncthreads();  // (S.neg and the slot arrays from every thread)
  if (blockIdx.x == 0) PSTAMP(2);
  for (int t = tid; t < 64; t += blockDim.x) {  // padding read branch-free by the scoring prologue: never a match
    P->oh_col[t] = 0;
    P->oh_val[t] = NAN;
  }
  // categorical mode: one-hot on the f16 matrix cores when every active dim has integer codes in
  // [0, 1024) and the one-hot width sum(max code + 1) fits OH_MAX_KC K-steps; else VALU matching.
  // One-hot positions: every dim's block starts at an even position (a padding position, level -1,
  // never matches) -- the sparse matrix-core kernel relies on adjacent pairs never spanning dims.
  // Thread 0 places the blocks (each dim's first level position), then one thread per dim fills its block.
  const int du = S.du;
  if (tid == 0) {
    int tot = 0;
    bool ok = true;
    for (int u = 0; u < du; ++u) {
      if (S.cm[u] < 0) {
        ok = false;
      } else {
        S.ohs[u] = (tot + 1) & ~1;
        tot = S.ohs[u] + S.cm[u] + 1;
      }
    }
    S.kc = (!S.exo && du > 0 && ok && 2 * tot <= 32 * OH_MAX_KC && tot <= 64) ? (2 * tot + 31) / 32 : 0;
    S.tot = tot;
  }
  __syncthreads();
  const int kc = S.kc;
  if (kc > 0) {
    for (int u = tid; u < du; u += blockDim.x) {
      int t = S.ohs[u];
      P->oh_start[u] = t;
      if (t > 0 && (u == 0 || t != S.ohs[u - 1] + S.cm[u - 1] + 1)) {  // the padding position before the block
        P->oh_dim[t - 1] = u;
        P->oh_level[t - 1] = -1;
      }
      for (int l = 0; l <= S.cm[u]; ++l, ++t) {
        P->oh_dim[t] = u;
        P->oh_level[t] = l;
        P->oh_col[t] = S.cd[u];
        P->oh_val[t] = (double)l;
      }
    }
  }
  if (threadIdx.x != 0) return;
  // (read back from LDS, not from the P just written: see above)
  const int dcp = S.dcp, dup = S.dup, has_neg = S.neg;
  if (S.exo) {  // no fp32 scoring: the acquisition re-scores every candidate
    P->hmode = 0;
    P->nsc = 0;
    // (within a bucket -- a single-level dim with h > 0 -- the table launch still runs: a well-formed f32 layout)
    P->chunk_floats = (dcp < 0 || dup < 0) ? 0 : chunk_floats(dcp, dup, 0, 0);
    return;
  }
  if (kc > 0) {
    P->kc = kc;
    P->oh_total = S.tot;
  }
  // continuous product on the f16 matrix cores (hi/lo split) when it has >= 8 dims (one full
  // 32-wide K-step; the C_j pieces ride in dims 0-2) and the categorical part is one-hot (or absent);
  // otherwise the exact f32 MFMA product.  |C_j| beyond the f16 range is caught after the table.
  const bool hm_ok = (du == 0 || kc > 0) && dcp >= 8;
  int hmode = (hm_ok && A.hm_allowed) ? 1 : 0;
  // the 32x32-tile kernel (hbx_score_h32.hip) in the buckets it is built for
  if (hmode && A.h32_allowed && h32_ok(nsc_of(dcp), h32_kp(kc), has_neg)) hmode = 2;
  P->hmode = hmode;
  P->nsc = nsc_of(dcp);
  P->chunk_floats = hmode == 2 ? h32_chunk_floats(nsc_of(dcp), h32_kp(kc), has_neg)
                               : (hmode ? h_chunk_floats(dcp, kc, has_neg) : chunk_floats(dcp, dup, kc, kc ? has_neg : 0));
  // the coarse pre-screen table (unsigned h32 KDEs): after the main table in the same buffer
  const bool co = hmode == 2 && !has_neg && A.co_allowed;
  P->coarse_chunk_floats = co ? h32c_chunk_floats(nsc_of(dcp), h32_kp(kc)) : 0;
  P->coarse_off = co ? (int32_t)(n_chunks_dev(n) * P->chunk_floats) : 0;
  if (blockIdx.x == 0) PSTAMP(3);
}

__global__ __launch_bounds__(256) void kde_params_kernel(PrepSet ps) {
  const PrepArgs& A = blockIdx.x ? ps.k[1] : ps.k[0];  // (no dynamic index into the kernel arguments)
  __shared__ ParamsScratch S;
  if (threadIdx.x == 0) *prep_counter(A.P) = 0;  // the table launch's block counter (finish by the last block)
  if (ps.pub.dst) prep_publish_rows(ps.pub, blockIdx.x ? 1 : 0, threadIdx.x, blockDim.x);
  kde_params_body(A, A.P, col_stats(A.P), S);
  // the published words acknowledged before the launch ends: the finishing blocks' flagged info words follow them
  if (ps.pub.dst) __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Fill the chunked observation table (layout in hbx_kde_impl.h).  X'_jc = s_c * (X_jc - mu_c),
// C_j = -sum_c X'_jc^2 + lb_sum - M0 (log2 units).  One thread per observation row (a serial walk over
// its dims), 64-thread blocks so a 1e4-row table spreads over ~150 CUs.  `hm` / `chunk_f` select the
// layout; |C_j| and |X'| maxima go to *cmax_acc / P->xmax.
// The one-hot positions observation row x matches, as a bit mask: position oh_start[u] + l for each active
// categorical dim u whose code is the integer l in [0, max code] -- exactly the positions t where
// x[oh_col[t]] == oh_val[t] (padding positions hold NaN: never), found with du loads instead of oh_total.
__device__ __forceinline__ uint64_t onehot_hits(const double* x, const KdeParams* P, bool ok) {
  uint64_t hit = 0;
  if (!ok) return hit;
  for (int u = 0; u < P->du; ++u) {
    const double v = x[P->cat_dim[u]];
    if (v >= 0.0 && v <= (double)P->cat_maxcode[u]) {
      const int l = (int)v;
      if (v == (double)l) hit |= 1ull << (P->oh_start[u] + l);
    }
  }
  return hit;
}

__device__ __forceinline__ void kde_table_body(const double* __restrict__ x, const KdeParams* __restrict__ P,
                                               KdeParams* __restrict__ Pw, float* __restrict__ table, int j,
                                               int hm, int chunk_f, float* cmax_acc, _Float16* hst) {
  // hst: this thread's LDS row (H32_ROW_MAX halves) where the h32 layout's dense slots are assembled
  // P: the parameters as read (an LDS copy); Pw: the global block, written (xmax, cmax / cmax2,
  // const_level) -- fields disjoint from every one read here
  const int n = P->n;
  const int nslots = ((n + OBS_CHUNK - 1) / OBS_CHUNK) * OBS_CHUNK;
  const bool ok = j < n;
  const bool slot = j < nslots;
  const int dc = P->dc, du = P->du, dcp = P->dc_pad, dup = P->du_pad;
  const int KP = kp_of(dcp);
  float* ch = table + (int64_t)(j / OBS_CHUNK) * chunk_f;
  const int jj = j % OBS_CHUNK;
  // hm: 0 = f32 layout, 1 = hmode (16x16 kernel), 2 = h32 (32x32 kernel, no chunk header)
  const int KTP = hm == 2 ? h32_ktp(P->nsc, h32_kp(P->kc), P->has_neg) : h_ktp(dcp, P->kc);
  _Float16* hrow = (_Float16*)(hm == 2 ? ch : ch + OBS_CHUNK) + jj * KTP;
  // the coarse pre-screen row (h32 KDEs with a coarse table; hbx_kde_impl.h): dense C pieces, ones, Xh
  _Float16* crow = (hm == 2 && P->coarse_off > 0 && slot)
                       ? (_Float16*)(table + P->coarse_off + (int64_t)(j / OBS_CHUNK) * P->coarse_chunk_floats) +
                             jj * h32c_ktp(P->nsc, h32_kp(P->kc))
                       : nullptr;
  double C = 0.0;
  // hmode rows are written 16 bytes (8 halves) at a time: two dims' h, l, h, l per store
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  h8 grp = {};
  const int nd32 = h32_nd(P->nsc);
  if (hm == 2) {
    for (int q = 0; q < 2 * nd32; ++q) *(h8*)(hst + 8 * q) = h8{};
    // eight dims at a time with no branch between them: their loads in flight together, then the stores and
    // the eight |X'| maxima (independent reductions); C accumulates in dim order as below
    for (int k0 = 0; k0 < dcp; k0 += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        const bool live = ok && k < dc;
        const double xv = x[live ? P->cont_dim[k] : 0];
        v[i] = live ? (float)(P->cont_scale[k] * (xv - P->center[k])) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        C -= (double)v[i] * (double)v[i];
        if (slot && k < dcp) {  // slots 6 + 3k: Xh, Xl, Xh
          const float vc = fminf(fmaxf(v[i], -60000.f), 60000.f);
          const _Float16 h = (_Float16)vc;
          const _Float16 l = (_Float16)(vc - (float)h);
          hst[6 + 3 * k] = h;
          hst[7 + 3 * k] = l;
          hst[8 + 3 * k] = h;
        }
      }
      // the eight |X'| maxima over the wave's 64 rows at once: every lane writes its eight, then lane (i, p)
      // takes dim i's rows 8p..8p+7 and the 8 lanes of dim i combine by lane exchanges (eight serial wave
      // reductions cost ~5k cycles per block); non-negative floats order as their bit patterns
      __shared__ __align__(16) uint32_t vab[8][64];
      const int ln = threadIdx.x & 63;
#pragma unroll
      for (int i = 0; i < 8; ++i) vab[i][ln] = __float_as_uint(fabsf(v[i]));
      __syncthreads();
      {
        const int i = ln >> 3, p8 = ln & 7;
        const uint4 q0 = *(const uint4*)&vab[i][8 * p8], q1 = *(const uint4*)&vab[i][8 * p8 + 4];
        uint32_t mx = max(max(max(q0.x, q0.y), max(q0.z, q0.w)), max(max(q1.x, q1.y), max(q1.z, q1.w)));
        mx = max(mx, lane_xor_u32(mx, 1, ln));
        mx = max(mx, lane_xor_u32(mx, 2, ln));
        mx = max(mx, lane_xor_u32(mx, 4, ln));
        if (p8 == 0 && k0 + i < dc) atomicMax((unsigned int*)&Pw->xmax[k0 + i], mx);
      }
      __syncthreads();  // (vab is rewritten by the next eight dims)
    }
  }
#pragma unroll 8
  for (int k = 0; k < (hm == 2 ? 0 : hm ? dcp : KP - 2); ++k) {
    float v = 0.f;
    if (ok && k < dc) v = (float)(P->cont_scale[k] * (x[P->cont_dim[k]] - P->center[k]));
    C -= (double)v * (double)v;
    if (slot) {
      if (hm) {
        const float vc = fminf(fmaxf(v, -60000.f), 60000.f);
        const _Float16 h = (_Float16)vc;
        const _Float16 l = (_Float16)(vc - (float)h);
        const int o = 4 * (k & 1);
        grp[o + 0] = h;
        grp[o + 1] = l;
        grp[o + 2] = h;
        grp[o + 3] = l;
        if (k & 1) *(h8*)(hrow + 4 * (k - 1)) = grp;
      } else {
        ch[(2 + k) * KROW + jj] = v;
      }
    }
    // |X'| maximum of the wave (non-negative floats order as their bit patterns)
    const uint32_t a = wave_reduce_dpp(__float_as_uint(fabsf(v)), OpMax());
    if ((threadIdx.x & 63) == 0 && k < dc) atomicMax((unsigned int*)&Pw->xmax[k], a);
  }
  if (blockIdx.x == 1) PSTAMP(14);
  const h8 z8 = {};
  if (hm == 1 && slot) {  // dc_pad is a multiple of 8: the dims filled whole groups
    for (int k = 4 * dcp; k < 32 * P->nsc; k += 8) *(h8*)(hrow + k) = z8;
    for (int k = 32 * (P->nsc + P->kc); k < KTP; k += 8) *(h8*)(hrow + k) = z8;
  }
  if (hm == 2 && slot)  // row padding past the index words (rows are 16-byte aligned, KTP % 8 == 0); the
    // parity block of a signed KDE is rewritten below
    for (int k = (16 * nd32 + 32 * h32_kp(P->kc) + 2 * h32_ixw(h32_kp(P->kc))) & ~7; k < KTP; k += 8)
      *(h8*)(hrow + k) = z8;
  if (P->kc == 0) {
    // the f32 layout's code block only: a matrix-core layout with kc == 0 has no active categorical dim (hm_ok),
    // and du_pad > 0 there means single-level dims alone -- writing their codes would overwrite row data
    if (hm == 0)
      for (int u = 0; u < dup; ++u) {
        const float v = (ok && u < du) ? (float)x[P->cat_dim[u]] : -2.0f;
        if (slot) ch[KP * KROW + jj * dup + u] = v;
      }
  } else if (slot && hm == 2) {
    // 2:4-compressed one-hot (h32 layout, hbx_kde_impl.h): per step s and group g (positions t0 = 32s + 4g
    // .. t0 + 3) the f16 hi / lo of delta_u for the observation's level in the pair (t0, t0+1) and in
    // (t0+2, t0+3), and the index nibble i0 | i1 << 2 (i0: 0 or 1, i1: 2 or 3); index dword ksp h + s
    // holds groups 4h..4h+3 of step s
    const int kp = h32_kp(P->kc);
    _Float16* cz = hrow + 16 * nd32;
    _Float16* cp = hrow + h32_par(P->nsc, kp);  // parity block (signed KDEs)
    _Float16* cc = crow ? crow + 16 * h32c_nd(P->nsc) : nullptr;
    const int ksp = h32_ksp(kp);
    if (blockIdx.x == 1) PSTAMP(17);
    // the matched position t of dim u (at most one per dim, never two in one pair: every dim's block starts at
    // an even position) puts delta_u's hi / lo (and the parity 1/2) at half t >> 1 of its part; every other
    // half is 0: zero-filled first, then one scattered half per matched dim (this thread's own row, in order)
    for (int q = 0; q < 2 * kp; ++q) {
      *(h8*)(cz + 8 * q) = z8;
      *(h8*)(cz + 16 * kp + 8 * q) = z8;
      if (cc) *(h8*)(cc + 8 * q) = z8;
      if (P->has_neg) *(h8*)(cp + 8 * q) = z8;
    }
    if (blockIdx.x == 1) PSTAMP(18);
    // eight dims at a time, every load of the eight issued before the first use (the positions matched are
    // those of onehot_hits: x[oh_col[t]] == oh_val[t])
    uint64_t hit = 0;
    for (int u0 = 0; u0 < (ok ? du : 0); u0 += 8) {
      int cd[8], cm[8], os[8];
      float dlt[8], ngf[8];
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {  // (indices < du + 8 <= 72: inside the HBX_MAX_D arrays)
        cd[i] = P->cat_dim[u0 + i];
        cm[i] = u0 + i < du ? P->cat_maxcode[u0 + i] : -1;
        os[i] = P->oh_start[u0 + i];
        dlt[i] = P->cat_delta[u0 + i];
        ngf[i] = P->cat_negf[u0 + i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = x[u0 + i < du ? cd[i] : 0];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!(v[i] >= 0.0 && v[i] <= (double)cm[i]) || v[i] != (double)(int)v[i]) continue;
        const int t = os[i] + (int)v[i], h = t >> 1;
        hit |= 1ull << t;
        const float dl = fminf(fmaxf(dlt[i], -60000.f), 60000.f);
        const float hi = (float)(_Float16)dl;
        cz[h] = (_Float16)hi;
        cz[16 * kp + h] = (_Float16)(fabsf(dl) < 60000.f ? dl - hi : 0.f);
        if (cc) cc[h] = (_Float16)hi;
        if (P->has_neg && ngf[i] != 0.f) cp[h] = (_Float16)0.5f;
      }
    }
    if (blockIdx.x == 1) PSTAMP(19);
    if (blockIdx.x == 1) PSTAMP(20);
    // index nibble of group g (positions t0 = 32 s + 4 g .. t0 + 3): i0 | i1 << 2 with i0 = 0 or 1, i1 = 2 or 3
    // (1 / 3 where the odd position of the pair matched); dword ksp h + s holds groups 4h..4h+3 of step s
    uint32_t iw[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int hh = q / ksp, st = q - hh * ksp, sh = 32 * st + 16 * hh;
      const uint32_t win = (st < kp && hh < 2 && sh < 64) ? (uint32_t)(hit >> sh) & 0xFFFFu : 0u;
      iw[q] = (st < kp && hh < 2) ? 0x8888u | ((win & 0xAAAAu) >> 1) : 0u;
    }
    for (int w = 0; w < (crow ? 2 : 1); ++w) {  // index words of the precise row, then of the coarse row
      uint32_t* ix = w == 0 ? (uint32_t*)(hrow + 16 * nd32 + 32 * kp) : (uint32_t*)(crow + 16 * h32c_nd(P->nsc) + 16 * kp);
      if (kp == 1) {  // dwords 2b + h, b = bit 4 of the row (bank spread of the kernel's b64 reads)
        const int b = (jj >> 4) & 1;
        for (int q = 0; q < 4; ++q) ix[q] = (q >> 1) == b ? iw[q & 1] : 0u;
      } else {
        for (int q = 0; q < 2 * ksp; ++q) ix[q] = iw[q];
      }
    }
  } else if (slot) {
    const int W = P->kc * 32;  // one-hot halves per observation
    _Float16* oh;
    _Float16* par;
    if (hm == 1) {
      oh = hrow + 32 * P->nsc;
      par = (_Float16*)(ch + OBS_CHUNK + OBS_CHUNK * KTP / 2) + jj * h_kpp(P->kc);
    } else {
      oh = (_Float16*)(ch + KP * KROW) + jj * W;
      par = (_Float16*)(ch + KP * KROW) + OBS_CHUNK * W + jj * W;
    }
    const uint64_t hit = onehot_hits(x, P, ok);
    h8 og = {}, pg = {};
#pragma unroll 8
    for (int k = 0; k < W; ++k) {
      const int t = k >> 1, p = k & 1;
      float v = 0.f, pv = 0.f;
      if (t < P->oh_total) {
        const int u = P->oh_dim[t];
        if ((hit >> t) & 1u) {
          const float dl = fminf(fmaxf(P->cat_delta[u], -60000.f), 60000.f);
          const float hi = (float)(_Float16)dl;
          v = (p == 0) ? hi : (fabsf(dl) < 60000.f ? dl - hi : 0.f);
          pv = (p == 0 && P->cat_negf[u] != 0.f) ? 1.f : 0.f;
        }
      }
      og[k & 7] = (_Float16)v;
      pg[k & 7] = (_Float16)pv;
      if ((k & 7) == 7) {  // W is a multiple of 32 and every row 16-byte aligned
        *(h8*)(oh + k - 7) = og;
        if (P->has_neg) *(h8*)(par + k - 7) = pg;
      }
    }
    if (hm == 1 && P->has_neg)
      for (int k = W; k < h_kpp(P->kc); k += 8) *(h8*)(par + k) = z8;
  }
  if (blockIdx.x == 1) PSTAMP(15);
  C += P->lb_sum - P->m0_log2;
  const float Cf = ok ? (float)C : -1e30f;
  if (slot) {
    if (hm) {
      if (hm == 1) ch[jj] = Cf;
      // C_j as three f16 pieces in the lo.lo slots 4c+3 of dims c = 0, 1, 2 (A side = 1 there);
      // padding rows get -60000, so their terms underflow to 0 (c_i <= 0, the rest of the row is 0;
      // h32: the shifted c_i stays below H32_CMAX = 30000)
      const float cv = ok ? fmaxf(Cf, -H_CMAX) : -H_CMAX;
      const _Float16 c0 = (_Float16)cv;
      const float r1 = cv - (float)c0;
      const _Float16 c1 = (_Float16)r1;
      const _Float16 c2 = (_Float16)(r1 - (float)c1);
      if (hm == 2) {  // slots 0-2: the C_j pieces; 3-5: 1 against the candidate's c_i pieces
        hst[0] = c0;
        hst[1] = c1;
        hst[2] = c2;
        hst[3] = hst[4] = hst[5] = (_Float16)1.f;
        for (int q = 0; q < 2 * nd32; ++q) *(h8*)(hrow + 8 * q) = *(const h8*)(hst + 8 * q);
        if (crow) {  // coarse dense slots: the same six, then Xh of continuous dim c at 6 + c; row padding
          const int ndc = h32c_nd(P->nsc), kpc = h32_kp(P->kc), ktpc = h32c_ktp(P->nsc, kpc);
          for (int q = 0; q < 2 * ndc; ++q) {
            h8 g;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int k = 8 * q + e;
              g[e] = k < 6 ? hst[k] : (k - 6 < dcp ? hst[6 + 3 * (k - 6)] : (_Float16)0.f);
            }
            *(h8*)(crow + 8 * q) = g;
          }
          for (int k = (16 * ndc + 16 * kpc + 2 * h32_ixw(kpc) + 7) & ~7; k < ktpc; k += 8) *(h8*)(crow + k) = z8;
        }
      } else {
        hrow[3] = c0;
        hrow[7] = c1;
        hrow[11] = c2;
      }
    } else {
      ch[0 * KROW + jj] = Cf;
      ch[1 * KROW + jj] = 1.f;
      if (jj < KROW - OBS_CHUNK)  // zero the pad columns of every k-row once per chunk
        for (int k = 0; k < KP; ++k) ch[k * KROW + OBS_CHUNK + jj] = 0.f;
    }
  }
  if (blockIdx.x == 1) PSTAMP(16);
  const uint32_t a = wave_reduce_dpp(__float_as_uint(ok ? fabsf(Cf) : 0.f), OpMax());
  if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)cmax_acc, a);
  if (j == 0)
    for (int q = 0; q < P->nconst; ++q) Pw->const_level[q] = x[P->const_dim[q]];
}

// f32-MFMA layout of an hmode KDE whose C_j left the f16 range of the three-piece split
__device__ __forceinline__ bool table_needs_rebuild(const KdeParams* P) { return P->hmode && !(P->cmax <= H_CMAX); }
// variant bit 8: at most 8 categorical slots and every active categorical dim's codes in [0, 3] -- the
// direct-difference ln-pdf pass then matches codes through two-bit fields and 256-entry tables (DD_LUT)
__device__ __forceinline__ int small_codes(const KdeParams* P) {
  if (P->du_pad != 4 && P->du_pad != 8) return 0;
  for (int u = 0; u < P->du; ++u)
    if (P->cat_maxcode[u] < 0 || P->cat_maxcode[u] > 3) return 0;
  return 1;
}

// Final mode of each KDE and its info record {variant, nan_all, unsupported, dc, du, nconst, dc_pad,
// du_pad}; variant (KdeVariant, hbx_kde_impl.h) selects the scoring kernel.  rebuild: the table needed its f32
// rebuild.
__device__ __forceinline__ int prep_variant(const KdeParams* P, int hmode, int coarse_off) {
  return KdeVariant{P->has_neg, P->kc, hmode != 0, P->exact_only, hmode == 2, hmode == 2 && coarse_off > 0,
                    small_codes(P)}.encode();
}
__device__ __forceinline__ void prep_finish_p(KdeParams* P, int32_t* info, bool rebuild) {
  if (rebuild) {
    P->hmode = 0;
    P->chunk_floats = chunk_floats(P->dc_pad, P->du_pad, P->kc, P->kc ? P->has_neg : 0);
    P->cmax = P->cmax2;
    P->coarse_off = 0;
  }
  info[0] = prep_variant(P, P->hmode, P->coarse_off);
  info[1] = P->nan_all;
  info[2] = P->unsupported;
  info[3] = P->dc;
  info[4] = P->du;
  info[5] = P->nconst;
  info[6] = P->dc_pad;
  info[7] = P->du_pad;
}
__device__ __forceinline__ void prep_finish_one(const PrepArgs& A, bool rebuild) { prep_finish_p(A.P, A.info, rebuild); }
// The same from R, the table launch's LDS copy of the block (every field read here is final before that
// launch), the rebuild's changes written to W, the record kept in vals: no global reads on the finishing
// block's path (cmax2: the rebuild's maximum, read by the caller)
__device__ __forceinline__ void prep_finish_lds(const KdeParams* R, KdeParams* W, int32_t* info, bool rebuild,
                                                float cmax2, int32_t (&vals)[8]) {
  int hmode = R->hmode, coarse = R->coarse_off;
  if (rebuild) {
    hmode = 0;
    coarse = 0;
    W->hmode = 0;
    W->chunk_floats = chunk_floats(R->dc_pad, R->du_pad, R->kc, R->kc ? R->has_neg : 0);
    W->cmax2 = cmax2;
    W->cmax = cmax2;
    W->coarse_off = 0;
  }
  vals[0] = prep_variant(R, hmode, coarse);
  vals[1] = R->nan_all;
  vals[2] = R->unsupported;
  vals[3] = R->dc;
  vals[4] = R->du;
  vals[5] = R->nconst;
  vals[6] = R->dc_pad;
  vals[7] = R->du_pad;
#pragma unroll
  for (int i = 0; i < 8; ++i) info[i] = vals[i];
}

// pass 0: the layout the parameter kernel chose; pass 1: the f32 rebuild where it is needed (every
// block of a KDE that needs none exits at once)
// The block's 64 observation rows are staged in LDS first (all loads in flight at once, coalesced
// within each row) when D <= 64; the per-dim walk then reads LDS instead of waiting on one dependent
// global load per dim.
// finish (pass 0 only): the KDE's last block to finish -- told by the counter its add returns, after every
// wave's stores and maxima atomics have been acknowledged -- rebuilds the table in the f32 layout when its
// C_j left the f16 range (rare: every row, in this block) and writes the final mode and the info record:
// the rebuild and finish launches saved.
#define TABLE_STAGE_D 64
// LDS row stride (halves) of the table launch's h32 rows: a 16-byte multiple >= H32_ROW_MAX whose dword count
// is not a multiple of 8 (112 halves = 56 dwords put lanes i and i + 8 on one bank: 8-way conflicts on the
// per-dim half stores; 120 = 60 dwords: 4-way)
#ifndef H32_ROW_STRIDE
#define H32_ROW_STRIDE 120
#endif
__global__ __launch_bounds__(64) void kde_table_kernel(PrepSet ps, float* table0, float* table1, int pass, int finish) {
  const bool second = ps.nk > 1 && (int)blockIdx.x >= ps.k[0].nblk_table;
  const PrepArgs& A = ps.k[second ? 1 : 0];
  KdeParams* P = A.P;
  const int j0 = (int)(blockIdx.x - (second ? ps.k[0].nblk_table : 0)) * 64;
  if (pass != 0 && !table_needs_rebuild(P)) return;
  if (blockIdx.x == 1) PSTAMP(8);
  // the parameter block is copied to LDS: loads from the global block the kernel also writes (atomics)
  // would be vector loads, one memory latency each along the per-dim walk
  // (every load issued before the first store: one memory latency for the whole block, not one per 1 KiB)
  constexpr int NPL = (int)((sizeof(KdeParams) + 15) / 16);
  __shared__ uint4 pl[NPL];
  for (int i0 = 0; i0 < NPL; i0 += 8 * 64) {
    uint4 t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = min(i0 + (int)threadIdx.x + 64 * q, NPL - 1);  // past the end: the last entry again
      t[q] = ((const uint4*)P)[i];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) pl[min(i0 + (int)threadIdx.x + 64 * q, NPL - 1)] = t[q];
  }
  __shared__ double xs[64 * (TABLE_STAGE_D + 1)];
  __shared__ __align__(16) _Float16 h32s[64 * H32_ROW_STRIDE];  // h32 rows assembled here
  const int D = A.D, n = A.n;
  const KdeParams* Pl = (const KdeParams*)pl;
  float* tab = second ? table1 : table0;
  // one block's 64 rows [r0, r0 + 64) of pass ps_: two inlined copies of the body, rows read from LDS
  // (every load a ds_read) or from global memory (a generic pointer would make each row read wait for the
  // outstanding table stores as well)
  auto rows64 = [&](int r0, int ps_) {
    const int j = r0 + threadIdx.x;
    auto run = [&](const double* x) {
      if (ps_ == 0)
        kde_table_body(x, Pl, P, tab, j, Pl->hmode, Pl->chunk_floats, &P->cmax, h32s + threadIdx.x * H32_ROW_STRIDE);
      else
        kde_table_body(x, Pl, P, tab, j, 0, chunk_floats(Pl->dc_pad, Pl->du_pad, Pl->kc, Pl->kc ? Pl->has_neg : 0),
                       &P->cmax2, h32s + threadIdx.x * H32_ROW_STRIDE);
    };
    if (D <= TABLE_STAGE_D) {
      const int DS = D | 1;  // odd row stride: the 64 threads' reads of one dim hit distinct banks
      __shared__ int64_t rs[64];
      __syncthreads();  // the parameter copy; the previous rows' readers done
      rs[threadIdx.x] = A.rows[j < n ? j : 0];
      __syncthreads();
      // 16 independent loads in flight per thread per batch (coalesced within each row); past the end
      // the last element is re-read and re-stored (same value, same place)
      const int tot = 64 * D;
      for (int e0 = 0; e0 < tot; e0 += 16 * 64) {
        double t[16];
        int at[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int e = min(e0 + q * 64 + (int)threadIdx.x, tot - 1);
          const int i = e / D, c = e - i * D;
          at[q] = i * DS + c;
          t[q] = A.X[rs[i] * (int64_t)D + c];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) xs[at[q]] = t[q];
      }
      __syncthreads();
      if (blockIdx.x == 1 && ps_ == 0) PSTAMP(9);
      run(xs + threadIdx.x * DS);
      if (blockIdx.x == 1 && ps_ == 0) PSTAMP(10);
    } else {
      __syncthreads();  // the parameter copy
      run(A.X + A.rows[j < n ? j : 0] * (int64_t)D);
    }
  };
  rows64(j0, pass);
  if (pass != 0 || !finish) return;
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's table stores and maxima atomics are done
  __syncthreads();
  if (blockIdx.x == 1) PSTAMP(11);
  __shared__ int last;
  if (threadIdx.x == 0) last = atomicAdd(prep_counter(P), 1) == A.nblk_table - 1;
  __syncthreads();
  if (!last) return;
  PSTAMP(12);
  // every block's |C_j| maximum is in (atomics at the device level; read past this CU's cache)
  const float cmax = __hip_atomic_load(&P->cmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool rebuild = Pl->hmode && !(cmax <= H_CMAX);
  if (rebuild) {
    for (int r0 = 0; r0 < A.nblk_table * 64; r0 += 64) rows64(r0, 1);
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float cm2 = rebuild ? __hip_atomic_load(&P->cmax2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    int32_t vals[8];
    prep_finish_lds(Pl, P, A.info, rebuild, cm2, vals);
    // the refit's output block to the host (hbx_kde_refit_sync): the rest went out with the parameter launch
    if (ps.pub.dst) prep_publish_vals(ps.pub, vals, second ? 1 : 0);
  }
  PSTAMP(13);
}

// Final mode of each KDE and its info record (the separate launch of hbx_kde_prepare's path)
__global__ void kde_prep_finish_kernel(PrepSet ps) {
  const int k = threadIdx.x;
  if (k >= ps.nk) return;
  const PrepArgs& A = k ? ps.k[1] : ps.k[0];
  prep_finish_one(A, table_needs_rebuild(A.P));
  if (ps.pub.dst) prep_publish_info(ps.pub, A, k);
}

static int64_t prep_table_blocks(int64_t n) { return (((n + OBS_CHUNK - 1) / OBS_CHUNK) * OBS_CHUNK + 63) / 64; }

int prep_args(PrepArgs* A, const double* X, int32_t D, const int64_t* rows, int32_t n, const int32_t* vartype,
              const double* bw, const int32_t* nlev, void* params, int32_t* info, int64_t table_floats_) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_UNSUPPORTED, "D=%d outside [1, %d]", D, HBX_MAX_D);
  if (n < 1) return hbx_fail(HBX_ERR_ARG, "KDE with n=%d observations", n);
  memset(A, 0, sizeof(*A));
  int dc = 0, du = 0;
  for (int d = 0; d < D; ++d) {
    if (vartype[d] != 0) {
      A->vt[d >> 5] |= 1u << (d & 31);
      ++du;
    } else {
      ++dc;
    }
  }
  int dcp, dup;
  bucket_dims(dc, du, &dcp, &dup);  // outside every bucket: an exact-only KDE (no table)
  if (table_floats_ < table_floats(n, dcp, dup))
    return hbx_fail(HBX_ERR_ARG, "table too small: %lld < %lld floats", (long long)table_floats_,
                    (long long)table_floats(n, dcp, dup));
  A->X = X;
  A->rows = rows;
  A->bw = bw;
  A->nlev = nlev;
  A->P = (KdeParams*)params;
  A->info = info;
  A->n = n;
  A->D = D;
  A->hm_allowed = hbx_switch_on("HBX_HMODE");    // 0: the f32-MFMA kernels everywhere (tests)
  A->h32_allowed = hbx_switch_on("HBX_H32");     // 0: the 16x16-tile hmode kernel instead of the 32x32 one
  A->co_allowed = hbx_switch_on("HBX_COARSE");   // 0: no coarse pre-screen table (the FAST instance scores)
  A->nblk_table = (dcp < 0 || dup < 0) ? 0 : (int32_t)prep_table_blocks(n);
  return HBX_OK;
}

// enqueue the preparation of ps.nk KDEs (no host synchronisation).  colstats_done: the fit wrote the column
// statistics already (refit_fit_colstats).  Every KDE with a table: the table launch's last block per KDE
// does the rare f32 rebuild and writes the final mode (3 launches; 5 before round 5)
int prep_launch(PrepSet& ps, float* table0, float* table1, hipStream_t s, bool colstats_done) {
  if (!colstats_done) {
    hipLaunchKernelGGL(kde_colstats_kernel, dim3(ps.nk * ps.k[0].D), dim3(256), 0, s, ps);
    HBX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kde_params_kernel, dim3(ps.nk), dim3(256), 0, s, ps);
  HBX_LAUNCH_CHECK();
  const bool all_tables = ps.k[0].nblk_table > 0 && (ps.nk < 2 || ps.k[1].nblk_table > 0);
  const unsigned tb = (unsigned)(ps.k[0].nblk_table + (ps.nk > 1 ? ps.k[1].nblk_table : 0));
  if (tb > 0) {
    hipLaunchKernelGGL(kde_table_kernel, dim3(tb), dim3(64), 0, s, ps, table0, table1, 0, all_tables ? 1 : 0);
    HBX_LAUNCH_CHECK();
  }
  if (!all_tables) {  // an exact-only KDE (no table) in the set: the separate passes
    if (tb > 0) {
      hipLaunchKernelGGL(kde_table_kernel, dim3(tb), dim3(64), 0, s, ps, table0, table1, 1, 0);
      HBX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(kde_prep_finish_kernel, dim3(1), dim3(64), 0, s, ps);
    HBX_LAUNCH_CHECK();
  }
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_table_floats(int32_t n, int32_t dc_pad, int32_t du_pad) { return table_floats(n, dc_pad, du_pad); }

int hbx_kde_bucket(int32_t dc, int32_t du, int32_t* dc_pad, int32_t* du_pad, int32_t* stride) {
  int a, b;
  bucket_dims(dc, du, &a, &b);
  if (a < 0 || b < 0) {  // outside every fp32 scoring bucket: exact-only KDEs
    *dc_pad = *du_pad = -1;
    *stride = 0;
    return hbx_fail(HBX_ERR_UNSUPPORTED, "no fp32 scoring kernel for %d continuous / %d categorical dims "
                    "(max 64 / 32): the KDE is exact-only (every candidate re-scored in fp64)", dc, du);
  }
  *dc_pad = a;
  *du_pad = b;
  *stride = table_stride(a, b);
  return HBX_OK;
}

// Build one KDE (good or bad) for scoring.  Host arrays: vartype[D] (0='c', 1='u'), bw[D], nlev[D].
// Device arrays: X[N][D] fp64 (rows of the whole budget), rows[n] int64 (this KDE's rows, in the
// reference's order).  Outputs: params (device, hbx_kde_param_bytes()), table (device fp32,
// hbx_kde_table_floats(n, dc_pad, du_pad) floats), info[8] (host): {variant, nan_all, unsupported, dc, du,
// nconst, dc_pad, du_pad}.  The host inputs go to the parameter buffer's staging area; the parameters
// are derived on the device (kde_params_kernel); one synchronisation for the info record.
int hbx_kde_prepare(const double* X, int32_t D, const int64_t* rows, int32_t n, const int32_t* vartype,
                    const double* bw, const int32_t* nlev, void* params, float* table, int64_t table_floats_,
                    int32_t* info, void* stream) {
  if (!X || !rows || !vartype || !bw || !nlev || !params || !table || !info)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_prepare: null pointer");
  char* stage = (char*)params + HBX_PARAM_STAGE;
  double* bw_d = (double*)stage;
  int32_t* nlev_d = (int32_t*)(stage + 8 * HBX_MAX_D);
  int32_t* info_d = nlev_d + HBX_MAX_D;
  PrepSet ps;
  memset(&ps, 0, sizeof(ps));
  ps.nk = 1;
  int rc = prep_args(&ps.k[0], X, D, rows, n, vartype, bw_d, nlev_d, params, info_d, table_floats_);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HBX_HIP(hipMemcpyAsync(bw_d, bw, 8 * (size_t)D, hipMemcpyHostToDevice, s));
  HBX_HIP(hipMemcpyAsync(nlev_d, nlev, 4 * (size_t)D, hipMemcpyHostToDevice, s));
  rc = prep_launch(ps, table, table, s);
  if (rc) return rc;
  HBX_HIP(hipMemcpyAsync(info, info_d, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HBX_HIP(hipStreamSynchronize(s));
  return HBX_OK;
}

}  // extern "C"

#ifdef PREP_STAMPS
extern "C" int hbx_debug_prep_stamps(unsigned long long* out) {
  HBX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(prep_stamps), sizeof(prep_stamps)));
  return HBX_OK;
}
#endif
