// hbx_exact.hip -- the fp64 evaluations of a prepared KDE on MI355X (gfx950), every kernel built on the reference's
// arithmetic in hbx_exact_impl.h in one unit (their shared helpers then compile in one context, as they always
// have): the acquisitions' exact re-score of a shortlist (kde_exact_kernel, kde_exact_combine_kernel, launched by
// acq_exact: hbx_acquire.h), KDEMultivariate.pdf (hbx_kde_pdf_exact), ln pdf in fp64 log space
// (hbx_kde_logpdf_exact), both over a listed subset for the ln-pdf contract (hbx_logpdf.hip), and numpy's exp.
#include "hbx_acquire.h"
#include "hbx_exact_impl.h"

// Exact re-score of the shortlist.  Small shortlists (<= EXACT_SPLIT_CAP): one work item per
// (candidate, KDE, 8192-buffer, unit) so one candidate spreads over many CUs; the unit sums go to
// `part` and kde_final combines them.  Larger: one item per (candidate, KDE), all units in turn.
// threads per block of the acquisition's exact re-score: one unit (<= 263 observations) per block; the 32 units of a
// buffer run on 32 CUs.  LANES = 1: one observation per thread, 256 threads (one wave per SIMD, six blocks per CU) --
// wherever the shortlist's length is not known to be short: batched and top-k acquisitions, and the unstaged single
// acquisition (small calls one after the other measured 6 % slower with the wide block: most lanes of short units
// idle, one block per CU).  LANES = 4: behind the staged acquisition's short tail, which runs at 1e8 pairs and
// more and shortlists a handful of candidates, so a block or less per CU, where the launch lasts as long as one
// thread's chain of restated-numpy exps: four adjacent lanes per observation, each with every fourth dim's factor
// (exact_unit_spread), 1024 threads, and a unit of <= 256 observations still takes one pass.
#define EXACT_ACQ_THREADS 256
#define EXACT_ACQ_LANES 4
// SCAN (a single acquisition of <= EXACT_SCAN_MAX candidates): no shortlist launch before this one -- every
// block restates kde_shortlist_kernel's predicate over the whole candidate set itself, in index order (a
// ballot prefix per wave), into its own LDS list; block 0 stores the list, its length and the zeroed marker
// count for the later kernels.  The final pick does not depend on the list's order (the atomics of the
// shortlist kernel give none).
// (EXACT_SCAN_MAX: hbx_acquire.h)
struct ExactScan {
  const float* lo;
  int64_t Nc;
  const uint32_t* U;
  const int32_t* flags;
  const int32_t* first1;
  int32_t* list;
  int32_t* count;
  int32_t* rescue_cnt;
};
template <bool SCAN, int LANES>
__global__ __launch_bounds__(EXACT_ACQ_THREADS * LANES) void kde_exact_kernel(
    const double* __restrict__ cand, int32_t D,
    const KdeParams* __restrict__ Pg, const double* __restrict__ Xg, const int64_t* __restrict__ rows_g,
    const KdeParams* __restrict__ Pb, const double* __restrict__ Xb, const int64_t* __restrict__ rows_b,
    const int32_t* __restrict__ list_in, const int32_t* __restrict__ count, int32_t nbuf, double* __restrict__ part,
    double* __restrict__ exact_l, double* __restrict__ exact_g, ExactScan sc) {
  __shared__ ExactShared sh;
  __shared__ int32_t slist[SCAN ? EXACT_SCAN_MAX : 1];
  constexpr int NT = EXACT_ACQ_THREADS * LANES;
  __shared__ int32_t swc[NT / 64];
  int cnt;
  const int32_t* list = list_in;
  if constexpr (SCAN) {
    const float u = hbx_ord2f(sc.U[0]);
    const bool all = (sc.flags[0] & 1) != 0;
    const int32_t f1 = sc.first1[0];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int64_t c0 = 0; c0 < sc.Nc; c0 += NT) {
      const int64_t i = c0 + threadIdx.x;
      bool in = false;
      if (i < sc.Nc) {
        const float l = sc.lo[i];
        in = (l == l && (all || l <= u)) || (int32_t)i == f1;
      }
      const uint64_t b = __ballot(in);
      if (lane == 0) swc[wv] = __popcll(b);
      __syncthreads();
      int off = base, tot = 0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) {
        off += w < wv ? swc[w] : 0;
        tot += swc[w];
      }
      if (in) slist[off + __popcll(b & ((1ull << lane) - 1))] = (int32_t)i;
      base += tot;
      __syncthreads();
    }
    cnt = base;
    list = slist;
    if (blockIdx.x == 0) {
      for (int k = threadIdx.x; k < cnt; k += NT) sc.list[k] = slist[k];
      if (threadIdx.x == 0) {
        *sc.count = cnt;
        if (sc.rescue_cnt) *sc.rescue_cnt = 0;
      }
    }
  } else {
    cnt = *count;
  }
  const bool split = cnt <= EXACT_SPLIT_CAP;
  const int per = split ? nbuf * PW_SPLIT_UNITS : 1;  // items per (candidate, KDE)
  const int64_t items = (int64_t)cnt * 2 * per;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t pk = item / per;  // (candidate, KDE)
    const int p = (int)(pk >> 1);
    const bool isl = pk & 1;
    const KdeParams* P = isl ? Pg : Pb;
    const double* X = isl ? Xg : Xb;
    const int64_t* rows = isl ? rows_g : rows_b;
    if (split) {
      const int r = (int)(item % per), b = r / PW_SPLIT_UNITS, u = r % PW_SPLIT_UNITS;
      const int n = P->n, c = b * PW_BUF;
      if (c >= n) continue;
      const int m = (n - c) < PW_BUF ? (n - c) : PW_BUF;
      int off, len;
      if (!pw_unit<PW_SPLIT_CUT>(m, u, &off, &len)) continue;
      exact_setup(P, D, cand + (int64_t)list[p] * D, &sh);
      double v;
      if constexpr (LANES > 1) v = exact_unit_spread<PW_SPLIT_LEVELS, LANES>(X, D, rows, P, c + off, len, &sh);
      else v = exact_unit<PW_SPLIT_LEVELS>(X, D, rows, P, c + off, len, &sh);
      if (threadIdx.x == 0) part[pk * per + r] = v;
    } else {
      exact_setup(P, D, cand + (int64_t)list[p] * D, &sh);
      const double v = exact_pdf(X, D, rows, P, &sh);
      if (threadIdx.x == 0) (isl ? exact_l : exact_g)[p] = v;
    }
    __syncthreads();
  }
}

// split mode: pdf of every (shortlisted candidate, KDE) from its unit sums; one thread each
__global__ __launch_bounds__(256) void kde_exact_combine_kernel(const KdeParams* __restrict__ Pg,
                                                                const KdeParams* __restrict__ Pb,
                                                                const int32_t* __restrict__ count, int32_t nbuf,
                                                                const double* __restrict__ part,
                                                                double* __restrict__ exact_l,
                                                                double* __restrict__ exact_g) {
  const int cnt = *count;
  if (cnt > EXACT_SPLIT_CAP) return;
  // one wave per (candidate, KDE)
  const int64_t pk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pk >= 2 * (int64_t)cnt) return;  // whole wave
  const bool isl = pk & 1;
  const int n = (isl ? Pg : Pb)->n;
  const double* us = part + pk * nbuf * PW_SPLIT_UNITS;
  double acc = 0.0;
  for (int c = 0, b = 0; c < n; c += PW_BUF, ++b) {
    const int m = (n - c) < PW_BUF ? (n - c) : PW_BUF;
    acc = acc + pw_combine_units_wave<PW_SPLIT_CUT>(m, us + b * PW_SPLIT_UNITS);
  }
  if ((threadIdx.x & 63) == 0) (isl ? exact_l : exact_g)[pk >> 1] = acc / (double)n;
}

// exact fp64 pdf of one KDE at every row of pts (grid-stride over points, one block per point)
// list (nullable): only the points list[0 .. *count), written at their own index; take_log: ln of the
// pdf, and only for KDEs the fp64 log-space kernel does not cover (negative factors, structural NaN)
__global__ __launch_bounds__(EXACT_THREADS) void kde_pdf_exact_kernel(const double* __restrict__ pts, int64_t Np,
                                                                      int32_t D, const KdeParams* __restrict__ P,
                                                                      const double* __restrict__ X,
                                                                      const int64_t* __restrict__ rows,
                                                                      double* __restrict__ out,
                                                                      const int32_t* __restrict__ list,
                                                                      const int32_t* __restrict__ count,
                                                                      int take_log) {
  __shared__ ExactShared sh;
  if (take_log && !(P->has_neg || P->nan_all || P->nconst)) return;
  const int64_t np = list ? (int64_t)*count : Np;
  for (int64_t p = blockIdx.x; p < np; p += gridDim.x) {
    const int64_t q = list ? (int64_t)list[p] : p;
    exact_setup(P, D, pts + q * D, &sh);
    const double v = exact_pdf(X, D, rows, P, &sh);
    if (threadIdx.x == 0) out[q] = take_log ? log(v) : v;
    __syncthreads();
  }
}

// ln pdf of one KDE at Np points in fp64 log space (one block per point): per observation j the
// log kernel product t_j = sum_c -(x_c - X_jc)^2 / (2 h_c^2) + sum_u ln K_u (SM:kernels.py:62-64,125
// with the constants pulled out), then ln pdf = logsumexp_j(t_j) - ln n - sum_c ln(h_c sqrt(2 pi)).
// No expansion and no fp64 underflow: accurate to ~1e-15 where the reference's own pdf is positive
// and still finite where the reference's fp64 pdf underflows to 0.  KDEs with negative categorical
// factors (bandwidth > 1 - 1/c) or structural NaNs are not handled here (NaN out): callers use the
// exact pdf there.  The mathematically exact counterpart of hbx_kde_logpdf's fp32 estimate.
__global__ __launch_bounds__(256) void kde_logpdf_exact_kernel(const double* __restrict__ pts, int64_t Np, int32_t D,
                                                              const KdeParams* __restrict__ P,
                                                              const double* __restrict__ X,
                                                              const int64_t* __restrict__ rows,
                                                              double* __restrict__ out,
                                                              const int32_t* __restrict__ list,
                                                              const int32_t* __restrict__ count) {
  __shared__ double c0[HBX_MAX_D], c1[HBX_MAX_D], xd[HBX_MAX_D];
  __shared__ int32_t cont[HBX_MAX_D];
  __shared__ double rm[4], rs[4];
  __shared__ double lconst;
  const int n = P->n;
  const int64_t np = list ? (int64_t)*count : Np;  // list: only those points, written at their own index
  for (int64_t pi = blockIdx.x; pi < np; pi += gridDim.x) {
    const int64_t p = list ? (int64_t)list[pi] : pi;
    const double* x = pts + p * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
      const double h = P->bw[d];
      const bool c = P->vartype[d] == 0;
      cont[d] = c;
      c0[d] = c ? 1.0 / ((h * h) * 2.) : log(1. - h);          // continuous: 1/(2h^2); categorical: ln(1-h)
      c1[d] = c ? 0.0 : log(h / (double)(P->nlev[d] - 1));     // categorical mismatch: ln(h/(c-1))
      xd[d] = x[d];
    }
    if (threadIdx.x == 0) {
      double lc = -log((double)n);
      for (int d = 0; d < D; ++d)
        if (P->vartype[d] == 0) lc -= log(P->bw[d]) + 0.91893853320467274178;  // ln(h sqrt(2 pi))
      lconst = lc;
    }
    __syncthreads();
    double m = -INFINITY, sm = 0.0;  // this thread's running logsumexp
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      const double* xr = X + rows[j] * (int64_t)D;
      double t = 0.0;
      for (int d = 0; d < D; ++d) {
        const double v = xr[d];
        if (cont[d]) {
          const double diff = v - xd[d];
          t -= diff * diff * c0[d];
        } else {
          t += (v == xd[d]) ? c0[d] : c1[d];
        }
      }
      if (t > m) {
        sm = sm * exp(m - t) + 1.0;
        m = t;
      } else if (t > -INFINITY) {
        sm += exp(t - m);
      } else if (t != t) {
        m = NAN;
      }
    }
    // block logsumexp of the (m, sm) pairs
    for (int o = 32; o > 0; o >>= 1) {
      const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(sm, o);
      const double mm = fmax(m, m2);
      if (m != m || m2 != m2) {
        m = NAN;
      } else if (mm > -INFINITY) {
        sm = (m > -INFINITY ? sm * exp(m - mm) : 0.0) + (m2 > -INFINITY ? s2 * exp(m2 - mm) : 0.0);
        m = mm;
      }
    }
    if ((threadIdx.x & 63) == 0) {
      rm[threadIdx.x >> 6] = m;
      rs[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double M = -INFINITY, Sx = 0.0;
      bool nan = false;
      for (int w = 0; w < 4; ++w) {
        if (rm[w] != rm[w]) nan = true;
        else if (rm[w] > -INFINITY) {
          const double mm = fmax(M, rm[w]);
          Sx = (M > -INFINITY ? Sx * exp(M - mm) : 0.0) + rs[w] * exp(rm[w] - mm);
          M = mm;
        }
      }
      out[p] = (nan || P->has_neg || P->nan_all || P->nconst) ? NAN : (M > -INFINITY ? M + log(Sx) + lconst : -INFINITY);
    }
    __syncthreads();
  }
}

int acq_exact(const KdePairRef& p, const double* cand, int64_t Nc, const AcqWs& a, bool scan, bool combine,
              hipStream_t s, bool wide) {
  if (scan && wide) return hbx_fail(HBX_ERR_ARG, "acq_exact: the wide re-score does not scan");
  const int nbuf = (int)((p.nmax + PW_BUF - 1) / PW_BUF);
  const ExactScan esc = scan ? ExactScan{a.lo, Nc, a.U, a.flags, a.first1, a.list, a.count, a.rescue} : ExactScan{};
  auto ek = wide   ? kde_exact_kernel<false, EXACT_ACQ_LANES>
            : scan ? kde_exact_kernel<true, 1>
                   : kde_exact_kernel<false, 1>;
  const dim3 threads(EXACT_ACQ_THREADS * (wide ? EXACT_ACQ_LANES : 1));
  hipLaunchKernelGGL(ek, dim3(EXACT_GRID), threads, 0, s, cand, p.D, p.Pg(), p.X_good, p.rows_good, p.Pb(), p.X_bad,
                     p.rows_bad, a.list, a.count, nbuf, a.part, a.exact_l, a.exact_g, esc);
  HBX_LAUNCH_CHECK();
  if (combine) {
    hipLaunchKernelGGL(kde_exact_combine_kernel, dim3((2 * EXACT_SPLIT_CAP + 3) / 4), dim3(256), 0, s, p.Pg(), p.Pb(),
                       a.count, nbuf, a.part, a.exact_l, a.exact_g);
    HBX_LAUNCH_CHECK();
  }
  return HBX_OK;
}

int hbx_logpdf_exact_listed(const double* cand, int64_t Nc, int32_t D, const KdeParams* P, const double* X,
                            const int64_t* rows, double* out, const int32_t* list, const int32_t* count,
                            bool per_point, hipStream_t s) {
  const unsigned grid = (unsigned)(Nc < EXACT_GRID ? Nc : EXACT_GRID);
  if (per_point) {
    hipLaunchKernelGGL(kde_logpdf_exact_kernel, dim3(grid), dim3(256), 0, s, cand, Nc, D, P, X, rows, out, list, count);
    HBX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kde_pdf_exact_kernel, dim3(grid), dim3(EXACT_THREADS), 0, s, cand, Nc, D, P, X, rows, out, list,
                     count, 1);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

// the exact pdf stages its per-observation terms in LDS: no global scratch is needed any more (the
// entry point keeps its scratch argument; 256 bytes keep callers' allocations non-empty)
int64_t hbx_kde_pdf_scratch_bytes(int64_t nmax) { return 256; }

// Exact fp64 pdf (reference arithmetic and operation order) of one prepared KDE at Np points
// (device fp64 [Np][D]) -> out (device fp64 [Np]).  KDEMultivariate.pdf as a batched GPU call.
int hbx_kde_pdf_exact(const double* pts, int64_t Np, int32_t D, const void* params, const double* X,
                      const int64_t* rows, int64_t n, double* out, void* scratch, int64_t scratch_bytes,
                      void* stream) {
  if (((!pts || !out) && Np > 0) || !params || !X || !rows || !scratch)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_pdf_exact: null");
  if (scratch_bytes < hbx_kde_pdf_scratch_bytes(n)) return hbx_fail(HBX_ERR_ARG, "pdf scratch too small");
  if (Np <= 0) return HBX_OK;
  const unsigned grid = (unsigned)(Np < EXACT_GRID ? Np : EXACT_GRID);
  hipLaunchKernelGGL(kde_pdf_exact_kernel, dim3(grid), dim3(EXACT_THREADS), 0, (hipStream_t)stream, pts, Np, D,
                     (const KdeParams*)params, X, rows, out, (const int32_t*)nullptr, (const int32_t*)nullptr, 0);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// ln pdf in fp64 log space (kde_logpdf_exact_kernel): the accurate log-domain value, NaN where the
// KDE has negative categorical factors or structural NaNs (use hbx_kde_pdf_exact there).
int hbx_kde_logpdf_exact(const double* pts, int64_t Np, int32_t D, const void* params, const double* X,
                         const int64_t* rows, double* out, void* stream) {
  if (((!pts || !out) && Np > 0) || !params || !X || !rows) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf_exact: null");
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf_exact: D=%d", D);
  if (Np <= 0) return HBX_OK;
  const unsigned grid = (unsigned)(Np < EXACT_GRID ? Np : EXACT_GRID);
  hipLaunchKernelGGL(kde_logpdf_exact_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pts, Np, D,
                     (const KdeParams*)params, X, rows, out, (const int32_t*)nullptr, (const int32_t*)nullptr);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// numpy's float64 exp (hbx_npexp.h) element-wise: the known-answer check of the exact re-score's exp
__global__ void np_exp_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = hbx_npexp::exp(x[i]);
}

int hbx_np_exp(const double* x, int64_t n, double* y, void* stream) {
  if ((!x || !y) && n > 0) return hbx_fail(HBX_ERR_ARG, "hbx_np_exp: null pointer");
  if (n <= 0) return HBX_OK;
  hipLaunchKernelGGL(np_exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, y);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

}  // extern "C"
