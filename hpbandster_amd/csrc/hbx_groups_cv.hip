// hbx_groups_cv.hip -- maximum-likelihood cross-validation ("cv_ml") bandwidths for every KDE of a grouped
// refit, searched on the device: one launch takes each (group, KDE) from the normal-reference bandwidths
// hbx_kde_fit left in bw_good / bw_bad to the bandwidths KDEMultivariate(bw='cv_ml') selects.
//
// Reference: SM:_kernel_base.py:267-332 (scipy.optimize.fmin from the normal-reference start, then the bounds),
// SM:kernel_density.py:126-160 (the objective, -sum_i ln L_i with leave-one-out L_i), SM:kernels.py:23-65,108-125
// (the Gaussian and Aitchison-Aitken kernels, the latter with the level count of the column WITHOUT row i).
//
// One workgroup per (group, KDE), the bad sets first (the long ones).  The Nelder-Mead search is sequential in its
// objective evaluations, so the block is the unit: the simplex ((D + 1) x D doubles) and its objective values live
// in LDS, the vertex arithmetic is done by one lane per dim with scipy's association, every decision is taken by
// all threads from the same LDS words (block-uniform control flow), and the objective itself uses the whole block:
//   lane = row i (rows beyond the block's lanes: further passes), L_i in a register of its own;
//   the j rows stream through LDS in chunks of 64, two buffers, one barrier per chunk, broadcast reads;
//   one exponential per pair, exp(-sum_c w_c (X_jc - X_ic)^2) with w_c = 1 / (2 h_c^2) held in scalar registers;
//   the differences are formed from the unscaled coordinates (scaling the rows first would leave the rounding of
//   x / h, not of the difference, in the exponent);
//   categorical factors are compares of the level values against two per-lane constants per dim, h / (c - 1) or
//   h / (c - 2) where row i's level occurs once in the column (a bit mask per row, found once before the search);
//   ln L_i = ln sum_j (...) - sum_c ln h_c - dc/2 ln 2 pi, summed over i in a fixed order (lane, wave, block).
// Everything is fp64: the search stops on objective differences of 1e-4 at values of 1e3 .. 1e4.  No global
// atomics; the results leave by ordinary stores.
#include <math.h>

#include "hbx_common.h"
#include "hbx_kde_impl.h"

#define CVG_THREADS 256
#define CVG_CHUNK 64
#define CVG_MAX_D 32

template <int DB>
struct CvgShared {
  double sim[(DB + 1) * DB];  // the simplex: vertex slot v at sim[v * DB], dims in the caller's order
  double fsim[DB + 1];
  double xbar[DB], xt[DB], xr[DB];
  // per slot (continuous dims first, then categorical, each in dim order) of the evaluation under way
  double w[DB], a1[DB], hq1[DB], hq2[DB];
  double buf[2][CVG_CHUNK * DB];
  double red[CVG_THREADS / 64];
  double lnorm, fval;
  int32_t ord[2][DB + 1];  // rank -> vertex slot, two copies (the sort writes the other one)
  int32_t slot_dim[DB];
  int32_t nlev[DB];
};

struct CvgKde {
  const double* Xs;    // the group's first row
  const int64_t* ord;  // the KDE's rows, local to the group
  uint32_t* single;    // per row: bit s set where the row's level occurs once in slot s's column
  int32_t n, D, dc;
};

__device__ __forceinline__ double cvg_uniform(double x) {  // a block-uniform value, into scalar registers
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}

// a before b in np.argsort's order of the objective values: ascending, NaN last
__device__ __forceinline__ bool cvg_lt(double a, double b) { return a == a && (b != b || a < b); }

// rows [j0, j0 + 64) of the KDE, slot order, into registers (0.0 past the KDE's rows and dims)
template <int DB>
__device__ __forceinline__ void cvg_fetch(const CvgKde& k, const int32_t* slot_dim, int j0, double (&v)[DB / 4]) {
#pragma unroll
  for (int q = 0; q < DB / 4; ++q) {
    const int e = (int)threadIdx.x + q * CVG_THREADS;
    const int j = j0 + e / DB, s = e % DB;
    v[q] = (j < k.n && s < k.D) ? k.Xs[k.ord[j] * (int64_t)k.D + slot_dim[s]] : 0.0;
  }
}

template <int DB>
__device__ __forceinline__ void cvg_store(double* buf, const double (&v)[DB / 4]) {
#pragma unroll
  for (int q = 0; q < DB / 4; ++q) buf[(int)threadIdx.x + q * CVG_THREADS] = v[q];
}

// body(rows, j0) for every chunk of 64 rows of the KDE, the rows staged in LDS; the next chunk is fetched
// while the body runs on this one
template <int DB, typename BODY>
__device__ __forceinline__ void cvg_sweep(const CvgKde& k, CvgShared<DB>* sh, BODY body) {
  double v[DB / 4];
  const int nch = (k.n + CVG_CHUNK - 1) / CVG_CHUNK;
  __syncthreads();  // the buffers' earlier readers are done
  cvg_fetch<DB>(k, sh->slot_dim, 0, v);
  cvg_store<DB>(sh->buf[0], v);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) cvg_fetch<DB>(k, sh->slot_dim, (c + 1) * CVG_CHUNK, v);
    body(sh->buf[c & 1], c * CVG_CHUNK);
    if (c + 1 < nch) cvg_store<DB>(sh->buf[(c + 1) & 1], v);
    __syncthreads();
  }
}

// row i of the KDE in slot order (row 0 for a lane past the KDE's rows: read, never used)
template <int DB>
__device__ __forceinline__ void cvg_row(const CvgKde& k, const int32_t* slot_dim, int i, double (&xi)[DB]) {
  const double* r = k.Xs + k.ord[i < k.n ? i : 0] * (int64_t)k.D;
#pragma unroll
  for (int s = 0; s < DB; ++s) xi[s] = s < k.D ? r[slot_dim[s]] : 0.0;
}

// before the search: per row the categorical slots where its level occurs exactly once in the column
template <int DB>
__device__ void cvg_singletons(const CvgKde& k, CvgShared<DB>* sh) {
  if (k.dc == k.D) return;  // (block-uniform)
  for (int i0 = 0; i0 < k.n; i0 += CVG_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    double xi[DB];
    int32_t cnt[DB];
    cvg_row<DB>(k, sh->slot_dim, i, xi);
#pragma unroll
    for (int s = 0; s < DB; ++s) cnt[s] = 0;
    cvg_sweep<DB>(k, sh, [&](const double* rows, int j0) {
      const int m = min(CVG_CHUNK, k.n - j0);
      for (int r = 0; r < m; ++r) {
#pragma unroll
        for (int s = 0; s < DB; ++s)
          if (s >= k.dc && s < k.D) cnt[s] += rows[r * DB + s] == xi[s];
      }
    });
    uint32_t mask = 0;
#pragma unroll
    for (int s = 0; s < DB; ++s)
      if (s >= k.dc && s < k.D && cnt[s] == 1) mask |= 1u << s;
    if (i < k.n) k.single[i] = mask;
  }
}

// f(h) = -sum_i ln L_i(h) at the bandwidths x[0 .. D) (LDS, the caller's dim order); every thread gets the value
// (not inlined: the search calls it from eight places)
template <int DB>
__device__ __attribute__((noinline)) double cvg_objective(const CvgKde& k, CvgShared<DB>* sh, const double* x) {
  const int tid = threadIdx.x;
  const int dc = k.dc, D = k.D;
  __syncthreads();  // x is written; the previous evaluation's constants are read
  if (tid < D) {
    const double h = x[sh->slot_dim[tid]];
    if (tid < dc) {
      sh->w[tid] = 1.0 / (2.0 * (h * h));
      sh->a1[tid] = log(h);
    } else {
      const int c = sh->nlev[tid];
      sh->a1[tid] = 1.0 - h;
      sh->hq1[tid] = h / (double)(c - 1);
      sh->hq2[tid] = h / (double)(c - 2);
    }
  }
  __syncthreads();
  if (tid == 0) {  // sum_c ln h_c + dc/2 ln 2 pi, in slot order
    double a = 0.0;
    for (int s = 0; s < dc; ++s) a = a + sh->a1[s];
    sh->lnorm = a + 0.5 * (double)dc * 1.8378770664093453;
  }
  double u1[DB];  // per slot, block-uniform: w_c of a continuous slot, 1 - h of a categorical one
#pragma unroll
  for (int s = 0; s < DB; ++s) u1[s] = cvg_uniform(s < dc ? sh->w[s] : s < D ? sh->a1[s] : 1.0);
  double lane_sum = 0.0;
  for (int i0 = 0; i0 < k.n; i0 += CVG_THREADS) {
    const int i = i0 + tid;
    double xi[DB], a0[DB];
    cvg_row<DB>(k, sh->slot_dim, i, xi);
    const uint32_t single = (dc < D && i < k.n) ? k.single[i] : 0u;
#pragma unroll
    for (int s = 0; s < DB; ++s) a0[s] = (s >= dc && s < D) ? ((single >> s) & 1u ? sh->hq2[s] : sh->hq1[s]) : 1.0;
    double L = 0.0;
    cvg_sweep<DB>(k, sh, [&](const double* rows, int j0) {
      const int m = min(CVG_CHUNK, k.n - j0);
      // four rows at a time: four independent exponent chains (rows past m hold zeros or earlier rows: masked)
      for (int r = 0; r < m; r += 4) {
        double e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < DB; ++s) {
          if (s < dc) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const double t = rows[(r + u) * DB + s] - xi[s];
              e[u] = fma(t * t, u1[s], e[u]);
            }
          }
        }
        double p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = exp(-e[u]);
#pragma unroll
        for (int s = 0; s < DB; ++s) {
          if (s >= dc && s < D) {
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = p[u] * (rows[(r + u) * DB + s] == xi[s] ? u1[s] : a0[s]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + r + u;
          if (r + u < m && j != i) L = L + p[u];
        }
      }
    });
    if (i < k.n) lane_sum = lane_sum + (log(L) - sh->lnorm);
  }
  // the sum over i in a fixed order: lanes of a wave pairwise, then the waves in order
  for (int o = 32; o > 0; o >>= 1) lane_sum = lane_sum + __shfl_xor(lane_sum, o);
  if ((tid & 63) == 0) sh->red[tid >> 6] = lane_sum;
  __syncthreads();
  if (tid == 0) {
    double a = sh->red[0];
    for (int v = 1; v < CVG_THREADS / 64; ++v) a = a + sh->red[v];
    sh->fval = -a;
  }
  __syncthreads();
  return sh->fval;
}

// np.argsort of the objective values (NaN last, equal values in position order) applied to the rank table
template <int DB>
__device__ __forceinline__ int cvg_sort(CvgShared<DB>* sh, int N, int cur) {
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid <= N) {
    const int me = sh->ord[cur][tid];
    const double fm = sh->fsim[me];
    int rank = 0;
    for (int q = 0; q <= N; ++q) {
      const double fq = sh->fsim[sh->ord[cur][q]];
      rank += q != tid && (cvg_lt(fq, fm) || (!cvg_lt(fm, fq) && q < tid));
    }
    sh->ord[cur ^ 1][rank] = me;
  }
  __syncthreads();
  return cur ^ 1;
}

// SM:_kernel_base.py:267-277, then the model's min_bandwidth as the fit applies it
__device__ __forceinline__ double cvg_bounds(double h, bool cont, double min_bw) {
  if (h < 0.0) h = 1e-10;
  if (!cont && h > 1.0) h = 1.0;
  return h < min_bw ? min_bw : h;
}

template <int DB>
__global__ __launch_bounds__(CVG_THREADS) void kde_cv_groups_kernel(
    const double* __restrict__ X, int32_t D, const int64_t* __restrict__ seg_off, int64_t B,
    const int64_t* __restrict__ order, const int64_t* __restrict__ n_good, const int64_t* __restrict__ n_bad,
    const int32_t* __restrict__ vartype, const int32_t* __restrict__ nlev_good, const int32_t* __restrict__ nlev_bad,
    double* __restrict__ bw_good, double* __restrict__ bw_bad, int32_t mode, int32_t max_evals,
    int32_t* __restrict__ status, double* __restrict__ objective, int32_t* __restrict__ evals_out,
    uint32_t* __restrict__ single, int64_t Ntot, double min_bw) {
  __shared__ CvgShared<DB> sh;
  const int tid = threadIdx.x;
  // the bad sets' (long) searches first, the good sets' filling the tail
  const int set = (int64_t)blockIdx.x < B ? 1 : 0;
  const int64_t b = set ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - B;
  const int64_t ns = set ? n_bad[b] : n_good[b];
  const int64_t s0 = seg_off[b], len = seg_off[b + 1] - s0;
  const int64_t out = b * 2 + set;
  if (ns <= 0 || ns > len || ns > INT32_MAX) {  // no model (hbx_kde_fit's rule): the bandwidths stay as they are
    if (tid == 0) {
      status[out] = HBX_CV_NO_MODEL;
      objective[out] = NAN;
      evals_out[out] = 0;
    }
    return;
  }
  double* bw = (set ? bw_bad : bw_good) + b * D;
  const int32_t* nlev = (set ? nlev_bad : nlev_good) + b * D;
  if (tid == 0) {  // slots: the continuous dims, then the categorical ones
    int dc = 0;
    for (int d = 0; d < D; ++d)
      if (vartype[d] == 0) sh.slot_dim[dc++] = d;
    int s = dc;
    for (int d = 0; d < D; ++d)
      if (vartype[d] != 0) sh.slot_dim[s++] = d;
    sh.ord[0][0] = dc;  // (handed to every thread below, then overwritten)
  }
  __syncthreads();
  CvgKde k;
  k.Xs = X + s0 * (int64_t)D;
  k.ord = order + s0 + (set ? len - ns : 0);
  k.single = single + (set ? Ntot : 0) + s0;
  k.n = (int32_t)ns;
  k.D = D;
  k.dc = __builtin_amdgcn_readfirstlane(sh.ord[0][0]);
  __syncthreads();
  const int N = D;
  bool ok = true;  // a start the search can use: every bandwidth finite and positive, level counts known
  if (tid < D) {
    const double h = bw[tid];
    sh.sim[tid] = h;
    sh.nlev[tid] = nlev[sh.slot_dim[tid]];
    ok = h > 0.0 && h < INFINITY && (vartype[tid] == 0 || nlev[tid] >= 1);
  }
  ok = __syncthreads_and(ok);
  cvg_singletons<DB>(k, &sh);
  if (mode == HBX_CV_EVAL) {
    const double f = cvg_objective<DB>(k, &sh, sh.sim);
    if (tid == 0) {
      status[out] = HBX_CV_CONVERGED;
      objective[out] = f;
      evals_out[out] = 1;
    }
    return;
  }
  if (!ok) {
    if (tid == 0) {
      status[out] = HBX_CV_NOT_SEARCHABLE;
      objective[out] = NAN;
      evals_out[out] = 0;
    }
    return;
  }
  // ---- scipy.optimize.fmin(xtol=1e-3, ftol=1e-4, maxiter=maxfun=max_evals), _optimize.py's Nelder-Mead ----
  int evals = 0;
  // one evaluation under the limit, which is checked first: false when the limit stops it
  auto ev = [&](const double* x, double* f) -> bool {
    if (evals >= max_evals) return false;
    *f = cvg_objective<DB>(k, &sh, x);
    ++evals;
    return true;
  };
  for (int v = tid; v <= N; v += CVG_THREADS) {
    sh.fsim[v] = INFINITY;
    sh.ord[0][v] = v;
  }
  if (tid < N) {  // vertex 1 + d: the start with component d scaled by 1.05 (0.00025 where it is 0)
    const double h = sh.sim[tid];
    for (int v = 1; v <= N; ++v) sh.sim[v * DB + tid] = (v - 1 == tid) ? (h != 0.0 ? (1.0 + 0.05) * h : 0.00025) : h;
  }
  for (int v = 0; v <= N; ++v) {
    double f;
    if (!ev(sh.sim + v * DB, &f)) break;
    if (tid == 0) sh.fsim[v] = f;
  }
  int cur = cvg_sort<DB>(&sh, N, 0);
  int it = 1;
  bool converged = false;
  // one iteration's body; false: the evaluation limit stopped it where it stood
  auto step = [&]() -> bool {
    const int32_t* ord = sh.ord[cur];
    const int best = ord[0], worst = ord[N];
    const double f0 = sh.fsim[best], fn1 = sh.fsim[ord[N - 1]], fw = sh.fsim[worst];
    double* xw = sh.sim + worst * DB;
    if (tid < N) {
      double a = sh.sim[best * DB + tid];
      for (int r = 1; r < N; ++r) a = a + sh.sim[ord[r] * DB + tid];
      const double xb = a / (double)N;
      sh.xbar[tid] = xb;
      sh.xr[tid] = (1.0 + 1.0) * xb - 1.0 * xw[tid];
    }
    auto take = [&](const double* x, double f) {  // sim[-1] = x, fsim[-1] = f
      if (tid < N) xw[tid] = x[tid];
      if (tid == 0) sh.fsim[worst] = f;
    };
    double fxr;
    if (!ev(sh.xr, &fxr)) return false;
    if (fxr < f0) {
      if (tid < N) sh.xt[tid] = (1.0 + 1.0 * 2.0) * sh.xbar[tid] - 1.0 * 2.0 * xw[tid];
      double fxe;
      if (!ev(sh.xt, &fxe)) return false;
      if (fxe < fxr) take(sh.xt, fxe);
      else take(sh.xr, fxr);
      return true;
    }
    if (fxr < fn1) {
      take(sh.xr, fxr);
      return true;
    }
    bool shrink = false;
    if (fxr < fw) {
      if (tid < N) sh.xt[tid] = (1.0 + 0.5 * 1.0) * sh.xbar[tid] - 0.5 * 1.0 * xw[tid];
      double fxc;
      if (!ev(sh.xt, &fxc)) return false;
      if (fxc <= fxr) take(sh.xt, fxc);
      else shrink = true;
    } else {
      if (tid < N) sh.xt[tid] = (1.0 - 0.5) * sh.xbar[tid] + 0.5 * xw[tid];
      double fxcc;
      if (!ev(sh.xt, &fxcc)) return false;
      if (fxcc < fw) take(sh.xt, fxcc);
      else shrink = true;
    }
    if (shrink) {
      for (int r = 1; r <= N; ++r) {
        double* xj = sh.sim + ord[r] * DB;
        if (tid < N) {
          const double x0 = sh.sim[best * DB + tid];
          xj[tid] = x0 + 0.5 * (xj[tid] - x0);
        }
        double f;
        if (!ev(xj, &f)) return false;
        if (tid == 0) sh.fsim[ord[r]] = f;
      }
    }
    return true;
  };
  while (evals < max_evals && it < max_evals) {
    const int32_t* ord = sh.ord[cur];
    bool small = true;  // max |sim[1:] - sim[0]| <= xtol and max |fsim[0] - fsim[1:]| <= ftol (a NaN fails)
    for (int e = tid; e < N * N; e += CVG_THREADS) {
      const int r = 1 + e / N, d = e % N;
      small = small && fabs(sh.sim[ord[r] * DB + d] - sh.sim[ord[0] * DB + d]) <= 1e-3;
    }
    if (tid >= 1 && tid <= N) small = small && fabs(sh.fsim[ord[0]] - sh.fsim[ord[tid]]) <= 1e-4;
    if (__syncthreads_and(small)) {
      converged = true;
      break;
    }
    if (step()) ++it;
    cur = cvg_sort<DB>(&sh, N, cur);
  }
  const int best = sh.ord[cur][0];
  if (tid < D) bw[tid] = cvg_bounds(sh.sim[best * DB + tid], vartype[tid] == 0, min_bw);
  if (tid == 0) {
    status[out] = converged ? HBX_CV_CONVERGED : HBX_CV_LIMIT;
    objective[out] = sh.fsim[best];
    evals_out[out] = evals;
  }
}

extern "C" {

// the rows' singleton masks of both sets: u32[2][N]
int64_t hbx_kde_cv_groups_workspace_bytes(int64_t N, int64_t B, int32_t D) {
  if (N < 0 || B < 0 || D < 1 || D > CVG_MAX_D || N > (INT64_MAX >> 4)) return -1;
  return 8 * N + 256;
}

int hbx_kde_cv_groups(const double* X, int64_t N, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                      const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const int32_t* nlev_good,
                      const int32_t* nlev_bad, double* bw_good, double* bw_bad, int32_t mode, int32_t max_evals,
                      int32_t* status, double* objective, int32_t* evals, void* workspace, int64_t ws_bytes,
                      void* stream, const hbx_rules* rules) {
  if (const int rc = hbx_rules_check("hbx_kde_cv_groups", rules)) return rc;
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !nlev_good || !nlev_bad || !bw_good || !bw_bad ||
      !status || !objective || !evals || !workspace)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: null pointer");
  if (D < 1) return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: D=%d", D);
  if (D > CVG_MAX_D)
    return hbx_fail(HBX_ERR_UNSUPPORTED, "hbx_kde_cv_groups: D=%d, the search holds at most %d dims", D, CVG_MAX_D);
  if (B < 0 || B > (1 << 30) || N < 0)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: B=%lld N=%lld", (long long)B, (long long)N);
  if (mode != HBX_CV_EVAL && mode != HBX_CV_ML) return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: mode %d", mode);
  if (max_evals < 1) return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: max_evals=%d", max_evals);
  if (((uintptr_t)X | (uintptr_t)seg_off | (uintptr_t)order | (uintptr_t)n_good | (uintptr_t)n_bad |
       (uintptr_t)bw_good | (uintptr_t)bw_bad | (uintptr_t)objective) & 7 ||
      ((uintptr_t)vartype | (uintptr_t)nlev_good | (uintptr_t)nlev_bad | (uintptr_t)status | (uintptr_t)evals |
       (uintptr_t)workspace) & 3)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: misaligned pointer");
  if (ws_bytes < hbx_kde_cv_groups_workspace_bytes(N, B, D))
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_cv_groups: workspace too small");
  if (B == 0) return HBX_OK;
  const double min_bw = rules ? rules->min_bandwidth : 0.0;
  const dim3 grid((unsigned)(2 * B)), block(CVG_THREADS);
#define CVG_LAUNCH(DB)                                                                                              \
  hipLaunchKernelGGL(kde_cv_groups_kernel<DB>, grid, block, 0, (hipStream_t)stream, X, D, seg_off, B, order, n_good, \
                     n_bad, vartype, nlev_good, nlev_bad, bw_good, bw_bad, mode, max_evals, status, objective,      \
                     evals, (uint32_t*)workspace, N, min_bw)
  if (D <= 8) CVG_LAUNCH(8);
  else if (D <= 16) CVG_LAUNCH(16);
  else CVG_LAUNCH(32);
#undef CVG_LAUNCH
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

}  // extern "C"
