// hbx_exact_impl.h -- the exact fp64 pdf in the reference's arithmetic (SM:_kernel_base.py:509-516: per-dim
// kernels, dim-ordered product, / prod(bw_c), numpy's pairwise sum, / n; numpy's exp bit for bit), shared by
// hbx_exact.hip (the acquisitions' re-score, the exact pdf entry points) and hbx_groups.hip (the grouped
// re-score).  Only the parameter type is a template argument: a KdeParams block, or any view with the
// members n, bw[d], vartype[d], nlev[d] and prod_bw_c (hbx_groups.hip's per-group view holds pointers into
// hbx_kde_fit's outputs).
#pragma once
#include "hbx_kde_impl.h"
#include "hbx_npexp.h"
#include "hbx_pairwise.h"

struct ExactShared {
  double dens[PW_UNIT_MAX];
  double nsum[PW_LEVELS][128];
  double usum[PW_UNITS];
  // per-dim constants of the reference kernels (SM:kernels.py:62-64,125): continuous -> (h*h)*2 in
  // c0, categorical -> 1-h in c0 and h/(c-1) in c1; the point's coordinates in xd
  double c0[HBX_MAX_D], c1[HBX_MAX_D], xd[HBX_MAX_D];
  int32_t cont[HBX_MAX_D];
};

// Per-dim constants + the point's coordinates into LDS (whole block).
template <typename PV>
__device__ void exact_setup(const PV* __restrict__ P, int32_t D, const double* __restrict__ x, ExactShared* sh) {
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const double h = P->bw[d];
    const bool c = P->vartype[d] == 0;
    sh->cont[d] = c;
    sh->c0[d] = c ? (h * h) * 2. : 1. - h;
    sh->c1[d] = c ? 0. : h / (double)(P->nlev[d] - 1);
    sh->xd[d] = x[d];
  }
  __syncthreads();
}

// Sum of the per-observation terms Kval.prod(1) / prod(bw_c) (SM:_kernel_base.py:509-516) over
// the observations [first, first+len) -- one unit of one buffer, pairwise order; whole block.
template <int LEVELS = PW_LEVELS, typename PV>
__device__ double exact_unit(const double* __restrict__ X, int32_t D, const int64_t* __restrict__ rows,
                             const PV* __restrict__ P, int first, int len, ExactShared* sh) {
  const double pbc = P->prod_bw_c;
  for (int j = threadIdx.x; j < len; j += blockDim.x) {
    const double* xr = X + rows[first + j] * (int64_t)D;
    double p = 1.0;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
      const double v = xr[d], xv = sh->xd[d];
      double k;
      if (sh->cont[d]) {
        const double diff = v - xv;
        k = HBX_INV_SQRT_2PI * hbx_npexp::exp(-(diff * diff) / sh->c0[d]);  // numpy's exp, bit for bit
      } else {
        k = (v == xv) ? sh->c0[d] : sh->c1[d];
      }
      p = (d == 0) ? k : p * k;
    }
    sh->dens[j] = p / pbc;
  }
  __syncthreads();
  return np_pairwise_block<LEVELS>(sh->dens, len, sh->nsum);
}

// The same unit sum with T adjacent lanes per observation (T a power of two <= 64; blockDim.x / T observations
// a pass): lane t of a group evaluates the factors of the dims t, T + t, ..., so a thread's chain of exps is D / T
// long instead of D, and every lane of the group multiplies the factors in dim order as they arrive -- the
// products ((k_0 k_1) k_2) ... of exact_unit, whichever lane evaluated k_d.  Same loads, same exp, same
// multiplications and division, same pairwise sum: same bits.  Whole block.
#define EXACT_SPREAD_ROUNDS 2
template <int LEVELS, int T, typename PV>
__device__ double exact_unit_spread(const double* __restrict__ X, int32_t D, const int64_t* __restrict__ rows,
                                    const PV* __restrict__ P, int first, int len, ExactShared* sh) {
  static_assert(T >= 1 && T <= 64 && (T & (T - 1)) == 0, "a group lies within one wave");
  const double pbc = P->prod_bw_c;
  const int t = threadIdx.x & (T - 1), nobs = blockDim.x / T;
  for (int j0 = 0; j0 < len; j0 += nobs) {  // (uniform trip count: every lane takes part in the shuffles)
    const int j = j0 + (int)threadIdx.x / T;
    const bool act = j < len;
    const double* xr = X + rows[first + (act ? j : 0)] * (int64_t)D;
    double p = 1.0;
    // EXACT_SPREAD_ROUNDS rounds of T dims at a time, fixed counts (the shuffles keep the compiler from unrolling a
    // loop of its own): the next rounds' coordinates are requested before this one's exps (past D: dim D - 1
    // again, a factor nobody multiplies), and a round past D evaluates nothing
    double vn[EXACT_SPREAD_ROUNDS];
#pragma unroll
    for (int q = 0; q < EXACT_SPREAD_ROUNDS; ++q) vn[q] = xr[q * T + t < D ? q * T + t : D - 1];
    for (int d0 = 0; d0 < D; d0 += T * EXACT_SPREAD_ROUNDS) {
      double v[EXACT_SPREAD_ROUNDS], k[EXACT_SPREAD_ROUNDS];
#pragma unroll
      for (int q = 0; q < EXACT_SPREAD_ROUNDS; ++q) {
        const int dn = d0 + (EXACT_SPREAD_ROUNDS + q) * T + t;
        v[q] = vn[q];
        vn[q] = xr[dn < D ? dn : D - 1];
      }
#pragma unroll
      for (int q = 0; q < EXACT_SPREAD_ROUNDS; ++q) {
        const int d = d0 + q * T + t < D ? d0 + q * T + t : D - 1;
        k[q] = 1.0;
        if (d0 + q * T < D) {  // (uniform)
          const double xv = sh->xd[d];
          if (sh->cont[d]) {
            const double diff = v[q] - xv;
            k[q] = HBX_INV_SQRT_2PI * hbx_npexp::exp(-(diff * diff) / sh->c0[d]);  // numpy's exp, bit for bit
          } else {
            k[q] = (v[q] == xv) ? sh->c0[d] : sh->c1[d];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < EXACT_SPREAD_ROUNDS; ++q) {
#pragma unroll
        for (int s = 0; s < T; ++s) {
          const double ks = __shfl(k[q], s, T);
          const int d = d0 + q * T + s;
          if (d < D) p = (d == 0) ? ks : p * ks;  // (uniform)
        }
      }
    }
    if (act && t == 0) sh->dens[j] = p / pbc;
  }
  __syncthreads();
  return np_pairwise_block<LEVELS>(sh->dens, len, sh->nsum);
}

// exact fp64 pdf of one KDE at the point staged by exact_setup, one block, all units in turn
template <typename PV>
__device__ double exact_pdf(const double* __restrict__ X, int32_t D, const int64_t* __restrict__ rows,
                            const PV* __restrict__ P, ExactShared* sh) {
  const int n = P->n;
  double acc = 0.0;  // np.add.reduce: identity 0.0, then one pairwise sum per 8192-element buffer
  for (int c = 0; c < n; c += PW_BUF) {
    const int m = (n - c) < PW_BUF ? (n - c) : PW_BUF;
    for (int u = 0; u < PW_UNITS; ++u) {
      int off, len;
      if (!pw_unit(m, u, &off, &len)) continue;
      const double v = exact_unit(X, D, rows, P, c + off, len, sh);
      if (threadIdx.x == 0) sh->usum[u] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) acc = acc + pw_combine_units(m, sh->usum);
  }
  return acc / (double)n;  // valid in thread 0
}
