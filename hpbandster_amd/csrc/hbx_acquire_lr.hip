// hbx_acquire_lr.hip -- single-pool acquisition by log ratio on MI355X (gfx950): the first index minimising
// s = ln g - ln l over one pool, with no floor (hbx_kde_acquire_lr, hbx_kde_acquire_bound_lr; bohb.py:124-169 with the
// score read in the log domain).  What hbx_kde_acquire_groups_batch_lr is to the grouped engine.
//
// The floored score max(f, g) / max(l, f) is exactly 1 wherever both densities lie under f -- nearly everywhere at 32
// dims -- and its strict argmin then returns candidate 0.  s still orders those candidates.  The call is an acquisition
// like hbx_kde_acquire: screen, shortlist, exact re-score, strict argmin, all on one stream; it does not form ln-pdfs of
// every candidate.
//
//   scoring    acq_plan / acq_score (hbx_acquire.h) as they are, unstaged, the rescue pass a launch of its own.  The
//              instance is decided by measurement (tools/bench_acquire_lr.py runs both): the coarse 32x32 one where the
//              pair has it; HBX_LR_COARSE=0, read per call, asks for fast without coarse (acq_plan's coarse_ok = false),
//              for models on which the coarse bound passes what the interval certifies (err < 0.9) and forces the pool.
//   combine    kde_combine_lr_kernel: per candidate the interval of s from both estimates (hbx_lr_interval.h, the
//              grouped route's derivation) into a.lo, the pool's bound U = min shi into a.U.  kde_combine_kernel's launch
//              shape and reduction; no tie at 1 (first1 stays INT32_MAX), no overflow flag.
//                  l not usable or may be 0, g not usable   forced: lo = -inf (always listed), never lowers U
//                  l or g certainly negative                lo = NaN: never listed, never re-scored
//                  g may be 0                               [-inf, +inf]: always listed, never lowers U
//                  otherwise                                lo = slo, shi enters U
//   shortlist  kde_shortlist_kernel / the re-score's scan form, and acq_exact with its unit sums combined: the
//              reference's fp64 pdfs bit for bit in a.exact_l / a.exact_g.  Exact-only pairs list everything.
//   ln         kde_lr_ln_kernel below: per shortlist entry and KDE
//                  L = log(p)            p a positive normal number (or +inf)
//                  L = NaN               p negative or NaN
//                  L = log(p)            p zero or subnormal, KDE with a negative match factor (-inf for 0)
//                  L = log-space value   p zero or subnormal, KDE without one: ln p in fp64 log space
//   final      kde_final_lr_kernel: s = L_g - L_l, the argmin by (hbx_d2ord(s), index) -- finite and -inf by value, +inf
//              behind them, NaN never picked; nothing with a score: index -1 --, the near set {s <= s_best + 1.0001 (rel +
//              rel_best)} with the log-space bounds added into rel, the record with score = s, the exact pdfs and
//              HBX_ACQ_LOG_RATIO, published like kde_final_kernel's (acq_publish, hbx_acq_impl.h).
//
// The log-space value (grp_logspace_ln's arithmetic and bound, hbx_groups_lr.hip, at 1e4 - 1e5 rows instead of 1e3):
//     t_j = sum_c -(x_c - X_jc)^2 / (2 h_c^2) + sum_u ([match] ln(1 - h_u) + [no match] ln(h_u / (c_u - 1)))
// by direct differences in fp64, ln p = ln sum_j exp(t_j) - ln n - sum_c ln h_c - dc ln sqrt(2 pi).  The KDE's rows
// stream through LDS in chunks of RC rows, two buffers, the next chunk's loads in flight while this one is evaluated;
// the loads are coalesced along the rows (no lane gathers a row of its own), the candidate's row and the per-dim
// constants are read once.  LPR adjacent lanes share a row (RC = 256 / LPR rows a chunk, LPR the smallest power of two
// at which a chunk fits its buffer: 2 at D = 32), each summing every LPR-th dim's term, then a butterfly adds the
// partial sums -- every term is <= 0, so every partial sum is at most |t| in magnitude, as the bound assumes.  The
// row's first lane keeps a running sum of exp2(t log2 e - m) against an INTEGER running maximum m, so every rescale is
// an exact ldexp; thread 0 merges the 256 partials in thread order, again by ldexp: no atomics on values, two runs give
// the same bytes.  A pair whose t is NaN or +inf makes the value NaN, as the reference's pdf is.
//     |ln p here - ln p| <= (D + 2) 2^-53 max|t| + (n + 256) 2^-52      (D >= dc + du; derivation: hbx_groups_lr.hip)
#include <float.h>
#include <string.h>

#include "hbx_acq_impl.h"
#include "hbx_acquire.h"
#include "hbx_host.h"
#include "hbx_lr_interval.h"

// ------------------------------------------------------------------------------------------
// the interval of s per candidate, U = min shi

__global__ __launch_bounds__(256) void kde_combine_lr_kernel(const KdeEst* __restrict__ el,
                                                             const KdeEst* __restrict__ eg, int64_t Nc, int negl,
                                                             int negg, float* __restrict__ lo,
                                                             uint32_t* __restrict__ U) {
  // COMBINE_SUB consecutive 256-candidate sub-blocks per block, every sub-block's loads issued first
  KdeEst ea[COMBINE_SUB], eb[COMBINE_SUB];
#pragma unroll
  for (int r = 0; r < COMBINE_SUB; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * COMBINE_SUB + r) * 256 + threadIdx.x;
    if (i < Nc) {
      ea[r] = el[i];
      eb[r] = eg[i];
    }
  }
  __shared__ float rh[COMBINE_SUB][4];
  float acc = INFINITY;  // thread 0: the sub-blocks' minima, lowered into U once per block
#pragma unroll
  for (int r = 0; r < COMBINE_SUB; ++r) {
    const int64_t blkr = (int64_t)blockIdx.x * COMBINE_SUB + r;
    if (blkr * 256 >= Nc) break;  // uniform
    const int64_t i = blkr * 256 + threadIdx.x;
    float h = INFINITY;
    if (i < Nc) {
      const LrIv v = lr_s_interval(grp_ln_interval(ea[r], negl != 0), grp_ln_interval(eb[r], negg != 0));
      float l = -INFINITY;  // forced: "not certified" takes the floored route's overflow flag's place, per candidate
      if (v.kind == LR_IV_NAN) l = NAN;
      if (v.kind == LR_IV_OK) {
        l = v.slo;
        h = v.shi;  // (+inf where g may be 0: never lowers U)
      }
      lo[i] = l;
    }
    for (int o = 32; o > 0; o >>= 1) h = fminf(h, __shfl_xor(h, o));
    if ((threadIdx.x & 63) == 0) rh[r][threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) acc = fminf(acc, fminf(fminf(rh[r][0], rh[r][1]), fminf(rh[r][2], rh[r][3])));
  }
  if (threadIdx.x == 0 && acc < INFINITY) {  // same-address atomics serialise: only where it can still lower U
    const uint32_t o = hbx_f2ord(acc);
    if (o < __hip_atomic_load(U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(U, o);
  }
}

// ------------------------------------------------------------------------------------------
// L per shortlist entry and KDE

#define LRL_T 256
#define LRL_BUF 4224                            // doubles per LDS stage: 128 rows of 33 (D = 32, odd stride)
#define LRL_NF ((LRL_BUF + LRL_T - 1) / LRL_T)  // a thread's loads per chunk at most

struct LrLnArgs {
  const double* cand;
  int32_t D;
  const KdeParams* P[2];  // [0] the good KDE (l), [1] the bad one (g)
  const double* X[2];
  const int64_t* rows[2];
  const int32_t* list;
  const int32_t* count;
  const double* exact[2];  // the exact pdfs per shortlist entry
  double* L;               // [2 p] L_l, [2 p + 1] L_g
  double* bnd;             // the log-space bound of each (0: no log-space value)
};

// One block per (shortlist entry, KDE), grid-stride from the device-side count (the grid is sized on the host from
// the pool: blocks past the count leave at once).  Two blocks per CU by LDS (76 KB each).
__global__ __launch_bounds__(LRL_T) void kde_lr_ln_kernel(LrLnArgs A) {
  __shared__ double buf[2][LRL_BUF];
  __shared__ double c0[HBX_MAX_D], c1[HBX_MAX_D], xd[HBX_MAX_D], lnh[HBX_MAX_D];
  __shared__ int32_t cont[HBX_MAX_D];
  __shared__ unsigned long long s_tmax;
  double* s_m = buf[0];  // the threads' partials, once the sweep has left the buffers
  double* s_s = buf[0] + LRL_T;
  const int tid = threadIdx.x;
  const int cnt = *A.count;
  const int D = A.D, DS = D | 1;
  int LPR = 1;
  while ((LRL_T / LPR) * DS > LRL_BUF) LPR <<= 1;  // (D <= 256: LPR <= 16, a row's lanes lie in one wave)
  const int RC = LRL_T / LPR;
  const int q = tid & (LPR - 1), r = tid / LPR;
  // this thread's elements of a chunk, e = tid + 256 k < RC D: (row in chunk) << 16 | dim, -1 past the chunk
  int pk[LRL_NF];
#pragma unroll
  for (int k = 0; k < LRL_NF; ++k) {
    const int e = tid + k * LRL_T;
    pk[k] = e < RC * D ? ((e / D) << 16) | (e % D) : -1;
  }
  for (int item = blockIdx.x; item < 2 * cnt; item += gridDim.x) {
    const int p = item >> 1, kd = item & 1;
    const double pdf = A.exact[kd][p];
    const KdeParams* __restrict__ P = A.P[kd];
    if (!(pdf >= 0.0 && pdf < DBL_MIN && !P->has_neg)) {  // (uniform) no log-space value is due
      if (tid == 0) {
        A.L[item] = (pdf != pdf || pdf < 0.0) ? NAN : log(pdf);  // (-0 -> -inf)
        A.bnd[item] = 0.0;
      }
      continue;
    }
    const double* __restrict__ x = A.cand + (int64_t)A.list[p] * D;
    const double* __restrict__ X = A.X[kd];
    const int64_t* __restrict__ rows = A.rows[kd];
    const int n = P->n;
    auto fetch = [&](int j0, double (&v)[LRL_NF]) {
#pragma unroll
      for (int k = 0; k < LRL_NF; ++k) {
        const int j = j0 + (pk[k] >> 16);
        v[k] = (pk[k] >= 0 && j < n) ? X[rows[j] * (int64_t)D + (pk[k] & 0xffff)] : 0.0;
      }
    };
    auto store = [&](double* b, const double (&v)[LRL_NF]) {
#pragma unroll
      for (int k = 0; k < LRL_NF; ++k)
        if (pk[k] >= 0) b[(pk[k] >> 16) * DS + (pk[k] & 0xffff)] = v[k];
    };
    double v[LRL_NF];
    fetch(0, v);
    // the per-dim constants (exact_setup's, the categorical ones as logs) and the candidate's row, once
    for (int d = tid; d < D; d += LRL_T) {
      const double h = P->bw[d];
      const bool c = P->vartype[d] == 0;
      cont[d] = c;
      c0[d] = c ? (h * h) * 2. : log(1. - h);  // (1 - h >= 0 here; ln 0 = -inf: a match contributes nothing)
      c1[d] = c ? 0. : log(h / (double)(P->nlev[d] - 1));
      xd[d] = x[d];
      lnh[d] = c ? log(h) : 0.0;
    }
    if (tid == 0) s_tmax = 0ull;
    store(buf[0], v);
    __syncthreads();
    double m = -INFINITY, s = 0.0, tmax = 0.0;
    bool bad = false;
    const int nch = (n + RC - 1) / RC;
    for (int c = 0; c < nch; ++c) {
      if (c + 1 < nch) fetch((c + 1) * RC, v);
      const double* row = buf[c & 1] + r * DS;
      double t = 0.0;
      for (int d = q; d < D; d += LPR) {
        const double xv = xd[d], o = row[d];
        if (cont[d]) {
          const double diff = o - xv;
          t -= (diff * diff) / c0[d];
        } else {
          t += (o == xv) ? c0[d] : c1[d];
        }
      }
      for (int o = LPR >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o);
      if (q == 0 && c * RC + r < n) {
        if (t != t || t == INFINITY) {
          bad = true;
        } else if (t > -INFINITY) {
          tmax = fmax(tmax, fabs(t));
          const double t2 = t * M_LOG2E, tc = ceil(t2);
          if (tc > m) {  // a new running maximum (integer): exact rescale
            s = ldexp(s, (int)fmax(m - tc, -2000.0));
            m = tc;
          }
          s += exp2(t2 - m);
        }
      }
      if (c + 1 < nch) store(buf[(c + 1) & 1], v);
      __syncthreads();
    }
    s_m[tid] = m;
    s_s[tid] = bad ? NAN : s;
    atomicMax(&s_tmax, (unsigned long long)__double_as_longlong(tmax));  // (non-negative doubles order as their bits)
    __syncthreads();
    if (tid == 0) {
      double M = -INFINITY, S = 0.0;
      for (int i = 0; i < LRL_T; ++i) M = fmax(M, s_m[i]);
      for (int i = 0; i < LRL_T; ++i) {
        const double si = s_s[i];
        if (si != si)
          S = NAN;
        else if (s_m[i] > -INFINITY)
          S += ldexp(si, (int)fmax(s_m[i] - M, -2000.0));
      }
      int dc = 0;
      double slh = 0.0;
      for (int d = 0; d < D; ++d)
        if (cont[d]) {
          slh += lnh[d];
          ++dc;
        }
      const double nrm = -log((double)n) - slh - (double)dc * (0.5 * log(2.0 * M_PI));
      A.L[item] = (S != S) ? NAN : (S > 0.0 ? (log2(S) + M) * M_LN2 + nrm : -INFINITY);
      A.bnd[item] = (double)(D + 2) * 0x1p-53 * __longlong_as_double((long long)s_tmax) + (double)(n + LRL_T) * 0x1p-52;
    }
    __syncthreads();  // (the buffers and the constants are free again)
  }
}

// ------------------------------------------------------------------------------------------
// the final argmin of one acquisition (256 threads): s = L_g - L_l over the shortlist, first index of the smallest key,
// the near set, the record

__global__ __launch_bounds__(256) void kde_final_lr_kernel(const int32_t* __restrict__ list,
                                                           const int32_t* __restrict__ count,
                                                           const double* __restrict__ exact_l,
                                                           const double* __restrict__ exact_g,
                                                           const double* __restrict__ L, const double* __restrict__ bnd,
                                                           const float* __restrict__ lo,
                                                           const int32_t* __restrict__ flags, int64_t index_base,
                                                           const KdeParams* __restrict__ Pg,
                                                           const KdeParams* __restrict__ Pb,
                                                           const KdeEst* __restrict__ el, const KdeEst* __restrict__ eg,
                                                           int32_t* __restrict__ near_list, AcqResult* __restrict__ res,
                                                           int32_t* __restrict__ stat, AcqResult* host_res, int32_t seq,
                                                           PickOut pick) {
  __shared__ uint64_t bk[256];
  __shared__ int64_t bi[256];
  __shared__ int32_t bp[256];
  __shared__ AcqResult rec_sh;
  __shared__ int32_t nnear, nls, nforce;
  const int cnt = *count;
  const int err_any = acq_pick_err_any(pick);
  if (threadIdx.x == 0) nnear = nls = nforce = 0;
  __syncthreads();
  auto score = [&](int p) { return L[2 * p + 1] - L[2 * p]; };
  // the absolute bound of one entry's s: both exact pdfs' relative bounds (hbx_acq_impl.h) and the log-space bounds
  auto rel = [&](int p) { return score_rel(Pg, Pb, el, eg, list[p]) + bnd[2 * p] + bnd[2 * p + 1]; };
  uint64_t key = ~0ull;  // every NaN has this key and never wins; +inf sorts behind every other score
  int64_t bidx = INT64_MAX;
  int32_t bpos = -1, ls = 0, nf = 0;
  for (int p = threadIdx.x; p < cnt; p += 256) {
    const uint64_t k = hbx_d2ord(score(p));
    const int64_t idx = list[p];
    if (k != ~0ull && (k < key || (k == key && idx < bidx))) {
      key = k;
      bidx = idx;
      bpos = p;
    }
    ls += (bnd[2 * p] > 0.0 ? 1 : 0) + (bnd[2 * p + 1] > 0.0 ? 1 : 0);
    nf += lo[idx] == -INFINITY ? 1 : 0;
  }
  if (ls) atomicAdd(&nls, ls);
  if (nf) atomicAdd(&nforce, nf);
  bk[threadIdx.x] = key;
  bi[threadIdx.x] = bidx;
  bp[threadIdx.x] = bpos;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      const uint64_t k2 = bk[threadIdx.x + w];
      const int64_t i2 = bi[threadIdx.x + w];
      if (k2 < bk[threadIdx.x] || (k2 == bk[threadIdx.x] && i2 < bi[threadIdx.x])) {
        bk[threadIdx.x] = k2;
        bi[threadIdx.x] = i2;
        bp[threadIdx.x] = bp[threadIdx.x + w];
      }
    }
    __syncthreads();
  }
  // the near set: every re-scored candidate the winner cannot be told apart from by these bounds (w = +inf: no
  // bound, near whatever s is)
  const int32_t wp = bp[0];
  double rb = 0.0, sb = NAN;
  if (wp >= 0) {
    sb = score(wp);
    rb = rel(wp);
    for (int p = threadIdx.x; p < cnt; p += 256) {
      const double s = score(p), w = 1.0001 * (rel(p) + rb);
      if (p == wp || (s < INFINITY && (w == INFINITY || s <= sb + w))) near_list[atomicAdd(&nnear, 1)] = list[p];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    AcqResult r;  // nothing with a score (an empty pool, every s NaN): the empty record, flagged like every other
    r.index = -1;
    r.score = r.pdf_l = r.pdf_g = NAN;
    r.shortlist = cnt;
    r.flags = *flags | (nnear > 1 ? HBX_ACQ_NEAR_TIE : 0) | HBX_ACQ_LOG_RATIO;
    r.near = nnear;
    r.rel = (float)rb;
    if (wp >= 0) {
      r.index = bi[0] + index_base;
      r.score = sb;
      r.pdf_l = exact_l[wp];
      r.pdf_g = exact_g[wp];
    }
    *res = r;
    rec_sh = r;
    stat[0] = nls;
    stat[1] = nforce;
  }
  acq_publish(&rec_sh, host_res, seq, pick, index_base, err_any);
}

// ------------------------------------------------------------------------------------------
// launch side

// HBX_LR_COARSE=0: score with the fast instance without the coarse 32x32 one.  The default is the coarse instance where
// the pair has one: measured at config #3 it certifies every candidate as well and the call is 1.2 - 1.7 ms against
// 1.9 - 2.1 (profiles/acquire_lr/README.md).  HBX_LR_SCAN=0: a shortlist launch of its own even for pools of
// <= EXACT_SCAN_MAX candidates (measured slower at 64).  Both read per call.
bool acq_lr_coarse() { return hbx_switch_on("HBX_LR_COARSE"); }

// CUs of the current device (asked once per device)
static int lr_cu_count() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

int acq_lr_ln(const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a, hipStream_t s) {
  const LrLnArgs la{cand, p.D, {p.Pg(), p.Pb()}, {p.X_good, p.X_bad}, {p.rows_good, p.rows_bad}, a.list, a.count,
                    {a.exact_l, a.exact_g}, a.lr_L, a.lr_bnd};
  const int64_t cap = 2 * (int64_t)lr_cu_count();  // two blocks per CU
  hipLaunchKernelGGL(kde_lr_ln_kernel, dim3((unsigned)(2 * Nc < cap ? 2 * Nc : cap)), dim3(LRL_T), 0, s, la);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

struct AcqLrCall {
  const char* who;
  const double* cand;
  int64_t Nc, index_base;
  void* workspace;
  int64_t ws_bytes;
  void *events, *stream;
  AcqResult* host_res;  // the bound call's publish target (acquire_impl's, hbx_kde.hip)
  int32_t seq;
  PickOut pick;
};

static int acquire_lr_impl(const void* pair, const AcqLrCall& c) {
  const KdePairRef* pp = acq_pair(c.who, pair);
  if (!pp) return HBX_ERR_ARG;
  const KdePairRef& p = *pp;
  const int64_t Nc = c.Nc;
  int rc = acq_check(c.who, p, c.cand, Nc, c.workspace);
  if (rc) return rc;
  const WsLayout w = ws_layout(Nc, p.nmax, 1, true);
  if ((size_t)c.ws_bytes < w.total)
    return hbx_fail(HBX_ERR_ARG, "workspace too small: %lld < %lld bytes", (long long)c.ws_bytes, (long long)w.total);
  AcqPlan plan;
  rc = acq_plan(p, true, &plan, acq_lr_coarse());
  if (rc) return rc;
  const AcqWs a(c.workspace, w);
  const hipStream_t s = (hipStream_t)c.stream;
  // unstaged (the staged acquisition prunes by the floor), splits for the pick, the rescue pass a launch of its own
  const ScoreRequest rq{c.cand, Nc, p.D, (hipEvent_t*)c.events, a.rescue, a.init(), p.nmax, false, s};
  ScoreResult sr;
  rc = acq_score(plan, p, a, rq, 0, &sr);
  if (rc) return rc;
  if (Nc > 0) {
    if (plan.exact_only) {
      rc = acq_exact_only_init(Nc, (uint32_t)Nc, a, s);
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL(kde_combine_lr_kernel, dim3((unsigned)((Nc + 256 * COMBINE_SUB - 1) / (256 * COMBINE_SUB))),
                         dim3(256), 0, s, a.el, a.eg, Nc, KdeVariant::decode(p.variant_good).has_neg,
                         KdeVariant::decode(p.variant_bad).has_neg, a.lo, a.U);
      HBX_LAUNCH_CHECK();
    }
    const bool scan = Nc <= EXACT_SCAN_MAX && hbx_switch_on("HBX_LR_SCAN");
    if (!scan) {
      rc = acq_shortlist(Nc, a, s);
      if (rc) return rc;
    }
    rc = acq_exact(p, c.cand, Nc, a, scan, true, s);
    if (rc) return rc;
    rc = acq_lr_ln(p, c.cand, Nc, a, s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(kde_final_lr_kernel, dim3(1), dim3(256), 0, s, a.list, a.count, a.exact_l, a.exact_g, a.lr_L,
                     a.lr_bnd, a.lo, a.flags, c.index_base, p.Pg(), p.Pb(), a.el, a.eg, a.near, a.res, a.lr_stat,
                     c.host_res, c.seq, c.pick);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_lr_workspace_bytes(int64_t Nc, int64_t nmax) { return (int64_t)ws_layout(Nc, nmax, 1, true).total; }

int hbx_kde_acquire_lr(const double* cand, int64_t Nc, int64_t index_base, const void* pair, void* workspace,
                       int64_t ws_bytes, void* events, void* stream) {
  return acquire_lr_impl(pair, {"hbx_kde_acquire_lr", cand, Nc, index_base, workspace, ws_bytes, events, stream,
                                nullptr, 0, PickOut{}});
}

int hbx_kde_acquire_bound_lr(const void* pair, const double* cand, int64_t Nc, int64_t index_base, void* workspace,
                             int64_t ws_bytes, const uint8_t* err, void* events, void* stream, void* rec_out,
                             double* row_out) {
  const char* who = "hbx_kde_acquire_bound_lr";
  if (!pair || !rec_out || Nc < 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_acquire_bound_lr: bad arguments");
  const KdePairRef& b = *(const KdePairRef*)pair;
  MappedBuf* mb = nullptr;
  int rc = hbx_mapped_acq(&mb);
  if (rc) return rc;
  char* pub = mb->p + PUB_OFF;
  const int32_t seq = mb->seq;
  const bool pick = err || row_out;
  rc = acquire_lr_impl(pair, {who, cand, Nc, index_base, workspace, ws_bytes, events, stream,
                              pick ? nullptr : (AcqResult*)pub, seq,
                              pick ? PickOut{cand, err, Nc, b.D, pub} : PickOut{}});
  if (rc) return rc;
  return acq_bound_wait(who, pub, seq, pick, b.D, Nc, index_base, (hipStream_t)stream, rec_out, row_out);
}

}  // extern "C"
