// hbx_sample.hip -- BOHB's candidate sampler on the GPU (bohb.py:133-147).
//
// Per candidate i: a good observation idx ~ U{0..n-1} (bohb.py:135), then per dim d of its row m:
//   continuous (levels[d] == 0): truncnorm.rvs(a=-m/bw, b=(1-m)/bw, loc=m, scale=bw_factor*bw)
//     (bohb.py:141).  The bounds are in units of bw while the scale is bw_factor*bw, so the sample
//     lies in [m - bw_factor*m, m + bw_factor*(1-m)] -- the reference's quirk, kept as is;
//   categorical (levels[d] = t): keep m with probability 1 - bw, else U{0..t-1} (bohb.py:143-146).
// The truncated normal is drawn by inversion, z = Phi^-1(p), p = Phi(a) + u (Phi(b) - Phi(a)) (Phi at
// the bounds in fp64; a > 0 is mirrored), Phi^-1 on the smaller tail min(p, 1 - p): in fp32 for
// min(p, 1 - p) >= 1e-6 (-sqrt(2) erfcinv(2 min(p, 1 - p)) by Giles' erfinv polynomials: within 4e-6 max(1, |z|)
// of scipy's ndtri there, 3e-7 the worst draw of the tests; a branch-free fp32 erfinv polynomial measured 3 %
// slower in round 5), and below 1e-6, where those polynomials extrapolate (1e-5 off at 1e-8, 3e-3 at 1e-10, 0.8 at
// 1e-16), from the fp64 AS 241 tail (norm_ppf_tail), to the same bound.  Data outside [0, 1] is supported: the
// bounds then both lie on one side of 0 and the whole interval [Phi(lo), Phi(hi)] can sit in a tail (m = -0.3,
// h = 0.05: z in [6, 26]), which is the fp64 path's case.
// Random numbers: Philox4x32-10 keyed by the seed (seed & 0xFFFFFFFF, seed >> 32); counter = (ctr & 0xFFFFFFFF,
// ctr >> 32, word, stream) with ctr = counter_base + i mod 2^64 of candidate i.  The datum index is
// (bits n) >> 64 of word 0xFFFFFFFF's bits = r[0] << 32 | r[1].  Dim d takes the 32-bit word r[slot] of the
// block at `word`, u = (r[slot] + 1/2) 2^-32:
//   pair k = d / 2 belongs to lane g = k % 4 as its q-th pair, q = k / 4:  word = g + 4 (q / 2), slot = 2 (q % 2) + d % 2
//   (in d alone: word = (d / 2) % 4 + 4 (d / 16), slot = 2 ((d / 8) % 2) + d % 2: period 16 in d, each word
//   serves 4 dims, words < 64 at HBX_MAX_D).  The 4 lanes per candidate are part of the stream's definition.
// A categorical dim keeps m when
// u < 1 - h and otherwise takes level floor(t (u - (1 - h)) / h) -- the conditional uniform of the same draw
// (h >= 1: always resampled, level floor(t u)).  The reference draws from numpy's global RNG, so parity with it
// is distributional (tests/test_gpu_sample.py); every draw is also checked against a host restatement of this
// header (tests/sampler_reference.py, tests/test_gpu_sample_draws.py: datum and categorical levels exactly, z to
// the bound above).
//
// One lane per (candidate, pair of dims), 4 lanes per candidate (kde_sample_pair_kernel).  Phi at the
// bounds comes from a per-model table when many candidates are drawn (hbx_kde_sample_table).
// hbx_norm_ppf keeps the fp64 inverse normal CDF (Wichura's AS 241) as a library function.
#include <math.h>

#include "hbx_common.h"
#include "hbx_philox.h"
#include <string.h>
#include <stdlib.h>

#define SAMPLE_BLOCK 256  // (DATUM_WORD and draw(): hbx_philox.h)

// Standardised bounds of a continuous dim around datum m, mirrored so that lo <= 0 side is used
// (a > 0 -> sample -z from [-b, -a]); false when scipy's a < b check fails.  rh = 1 / h: the bounds are
// within an ulp or two of scipy's -m / h, (1 - m) / h (a distributional difference of nothing), and the
// domain check agrees exactly (h = 0: +-inf, or NaN where m is 0 or 1, as with the divisions).
__device__ __forceinline__ bool tn_bounds(double m, double rh, double* lo, double* hi, bool* flip) {
  const double a = -m * rh, b = (1.0 - m) * rh;
  if (!(a < b)) return false;
  *flip = a > 0.0;
  *lo = *flip ? -b : a;
  *hi = *flip ? -a : b;
  return true;
}

// Phi^-1(p), p in (0, 1), in double precision: Wichura's algorithm AS 241 (PPND16, Applied Statistics
// 37, 1988) -- a 7/7 rational in (0.180625 - (p-0.5)^2) for |p - 0.5| <= 0.425, else in
// sqrt(-log(min(p, 1-p))) on two ranges; relative error ~1e-16 (<= 1.1e-15 against scipy's ndtri over
// 2.4e5 probe points, including 1e-300 and 1 - 1e-10).  One log and one sqrt in the tails, no erfc /
// exp refinement step (the former fp32 guess + fp64 Halley step spent most of the sampler's time in
// ocml's fp64 normcdf and exp).
__device__ __forceinline__ double as241_poly(const double (&c)[8], double x) {
  double r = c[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) r = fma(r, x, c[k]);
  return r;
}

// Phi^-1(r) for a tail probability r = min(p, 1 - p) < 0.075 (the two outer ranges of AS 241): <= 0.  Out of line:
// the sampler calls it on a branch almost no lane takes, and inlined there it raised the table instance from 44 to
// 120 VGPRs (8 to 4 waves per SIMD) and a 1e6 x 32 launch from 0.120 to 0.140 ms; as a call, 52 VGPRs and 0.120 ms.
__device__ __noinline__ double norm_ppf_tail(double r) {
  constexpr double C[8] = {1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0,
                           3.64784832476320460504e0, 1.27045825245236838258e0, 2.41780725177450611770e-1,
                           2.27238449892691845833e-2, 7.74545014278341407640e-4};
  constexpr double D[8] = {1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
                           1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4,
                           1.05075007164441684324e-9};
  constexpr double E[8] = {6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0,
                           2.96560571828504891230e-1, 2.65321895265761230930e-2, 1.24266094738807843860e-3,
                           2.71155556874348757815e-5, 2.01033439929228813265e-7};
  constexpr double F[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                           7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7,
                           2.04426310338993978564e-15};
  r = sqrt(-log(r));
  double v;
  if (r <= 5.0) {
    r -= 1.6;
    v = as241_poly(C, r) / as241_poly(D, r);
  } else {
    r -= 5.0;
    v = as241_poly(E, r) / as241_poly(F, r);
  }
  return -v;
}

__device__ __forceinline__ double norm_ppf(double p) {
  constexpr double A[8] = {3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3,
                           1.3731693765509461125e+4, 4.5921953931549871457e+4, 6.7265770927008700853e+4,
                           3.3430575583588128105e+4, 2.5090809287301226727e+3};
  constexpr double B[8] = {1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
                           2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4,
                           5.2264952788528545610e+3};
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * as241_poly(A, r) / as241_poly(B, r);
  }
  const double v = norm_ppf_tail(q < 0.0 ? p : 1.0 - p);  // 1 - p: exact for p >= 0.5 (Sterbenz)
  return q < 0.0 ? v : -v;
}

__global__ void norm_ppf_kernel(const double* __restrict__ p, int64_t n, double* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = norm_ppf(p[i]);
}

// Per (datum j, dim d) constants of the continuous dims: {Phi(lo), Phi(hi)} (NaN pair: domain error;
// the sign of Phi(hi) - Phi(lo) is unused).  A property of the good KDE, computed once per model when
// many candidates are drawn from it (the two normcdf calls dominate a draw otherwise).
__global__ __launch_bounds__(SAMPLE_BLOCK) void kde_sample_table_kernel(
    const double* __restrict__ X, int32_t D, const int64_t* __restrict__ rows, int64_t n,
    const double* __restrict__ bw, const int32_t* __restrict__ levels, double2* __restrict__ tab) {
  const int64_t total = n * (int64_t)D;
  for (int64_t e = (int64_t)blockIdx.x * SAMPLE_BLOCK + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * SAMPLE_BLOCK) {
    const int64_t j = e / D;
    const int d = (int)(e - j * D);
    double2 r = make_double2(0.0, 0.0);
    if (levels[d] == 0) {
      double lo, hi;
      bool flip;
      if (tn_bounds(X[rows[j] * (int64_t)D + d], 1.0 / bw[d], &lo, &hi, &flip))
        r = make_double2(normcdf(lo), normcdf(hi));
      else
        r = make_double2(NAN, NAN);
    }
    tab[e] = r;
  }
}

// z = Phi^-1(p) on the smaller tail in fp32, p = Phi(lo) + u (Phi(hi) - Phi(lo)) in fp64, clamped to [lo, hi]
// erfcinv(t), t in (0, 1], in single precision without the library's branches: M. Giles' single-precision erfinv
// polynomials ("Approximating the erfinv function", GPU Computing Gems Jade, 2011; relative error ~4e-7) at
// x = 1 - t, with w = -ln((1 - x)(1 + x)) formed from t itself (t (2 - t): exact in the tail where 1 - t rounds)
__device__ __forceinline__ float fast_erfcinvf(float t) {
  float w = -__logf(t * (2.0f - t));
  float p;
  if (w < 5.0f) {
    w = w - 2.5f;
    p = 2.81022636e-08f;
    p = fmaf(p, w, 3.43273939e-07f);
    p = fmaf(p, w, -3.5233877e-06f);
    p = fmaf(p, w, -4.39150654e-06f);
    p = fmaf(p, w, 0.00021858087f);
    p = fmaf(p, w, -0.00125372503f);
    p = fmaf(p, w, -0.00417768164f);
    p = fmaf(p, w, 0.246640727f);
    p = fmaf(p, w, 1.50140941f);
  } else {
    w = sqrtf(w) - 3.0f;
    p = -0.000200214257f;
    p = fmaf(p, w, 0.000100950558f);
    p = fmaf(p, w, 0.00134934322f);
    p = fmaf(p, w, -0.00367342844f);
    p = fmaf(p, w, 0.00573950773f);
    p = fmaf(p, w, -0.0076224613f);
    p = fmaf(p, w, 0.00943887047f);
    p = fmaf(p, w, 1.00167406f);
    p = fmaf(p, w, 2.83297682f);
  }
  return p * (1.0f - t);
}

// Giles' polynomial is fitted for float erfinv, w <~ 17 (min(p, 1 - p) ~ 1e-8), and extrapolates beyond.  Below
// TN_TAIL_T = 2e-6f (min(p, 1 - p) < 1e-6, w > 12.4: a margin, the polynomial's error already grows there) z comes
// from the fp64 AS 241 tail of min(p, 1 - p) itself -- one log and one sqrt on a branch that a draw from data in
// [0, 1] takes about once in 1e6, and every draw of a datum far outside [0, 1] takes.
#define TN_TAIL_T 2e-6f
__device__ __forceinline__ double tn_invert_f32(double plo, double phi, double lo, double hi, double u) {
  const double p = fma(u, phi - plo, plo);
  const bool up = p > 0.5;
  const double pm = up ? 1.0 - p : p;  // min(p, 1 - p)
  const float t = (float)(2.0 * pm);   // in (0, 1]
  double zt;                           // Phi^-1(min(p, 1 - p)) <= 0
  if (t < TN_TAIL_T)
    zt = norm_ppf_tail(pm);
  else
    zt = (double)(-1.41421356237309505f * fast_erfcinvf(t));
  // (the library's erfcinvf: the same draws in distribution, 0.126 instead of 0.113 ms per 1e6 x 32 launch)
  const double z = up ? -zt : zt;
  return fmin(fmax(z, lo), hi);
}

// One draw of dim d of a candidate whose datum row is xr from the 32-bit uniform word w0.
// TAB: the Phi table is given (one instance each way: the table instance carries no inlined normcdf)
template <bool TAB>
__device__ __forceinline__ double sample_dim(const double* __restrict__ xr, int d, int32_t idx, int32_t D,
                                             const double* __restrict__ bw, const double* __restrict__ rbw,
                                             const int32_t* __restrict__ levels,
                                             const double2* __restrict__ tab, double bw_factor, uint32_t w0,
                                             bool* derr) {
  const double m = xr[d];
  const double h = bw[d];
  const int t = levels[d];
  const double u = ((double)w0 + 0.5) * 0x1p-32;  // open (0, 1)
  if (t != 0) {  // keep m with probability 1 - h, else a uniform level: both from the one uniform
    const double thr = 1.0 - h;
    if (u < thr) return m;
    const double v = thr > 0.0 ? (u - thr) * rbw[d] : u;  // ~uniform on [0, 1) given the resample (1 / h: LDS)
    const int lv = (int)(v * (double)t);
    return (double)(lv < t ? lv : t - 1);
  }
  double lo, hi;
  bool flip;
  if (!tn_bounds(m, rbw[d], &lo, &hi, &flip)) {  // scipy's argcheck fails: the reference call raises
    *derr = true;
    return NAN;
  }
  double plo, phi;
  if constexpr (TAB) {
    const double2 p = tab[(int64_t)idx * D + d];
    plo = p.x;
    phi = p.y;
  } else {
    plo = normcdf(lo);
    phi = normcdf(hi);
  }
  const double z = tn_invert_f32(plo, phi, lo, hi, u);
  return fma(bw_factor * h, flip ? -z : z, m);
}

// The draws with one (candidate, pair of dims) per lane: L = SAMPLE_LPC lanes per candidate, lane g of the
// group takes the pairs g, g + L, ...  A candidate's datum row and Phi-table row are then read by its L lanes
// as contiguous 16-byte pieces and its output row is written as contiguous 16-byte stores (a lane-per-
// candidate layout, 8-9 % slower with the same draws, was removed in round 5).  One Philox block per lane and
// two pairs (word g + L i for pairs g + 2 L i and g + L + 2 L i): the block's four words are the four dims'
// uniforms -- a categorical dim takes both its keep-or-resample decision and its level from its uniform --
// so a candidate costs D / 4 blocks (D before round 5: two words per dim, the generator half the work).
// Dim types and bandwidths vary across the lanes (loaded per lane; the categorical branch is the cheap
// one): with 4 lanes a 24c + 8u candidate's 16 pairs take three all-continuous steps and one all-categorical
// step, where 8 lanes ran a mixed step through both branches.  Counter (candidate, word, stream): the draws
// do not depend on the launch shape.
#ifndef SAMPLE_LPC
#define SAMPLE_LPC 4  // lanes per candidate (8: 0.130 ms, 2: 0.196 ms per 1e6 x 32 launch against 0.119 ms; lib_ab)
#endif
template <bool TAB>
__global__ __launch_bounds__(256) void kde_sample_pair_kernel(
    const double* __restrict__ X, int32_t D, const int64_t* __restrict__ rows, int64_t n,
    const double* __restrict__ bw, const int32_t* __restrict__ levels, const double2* __restrict__ tab,
    double bw_factor, uint64_t seed, uint64_t counter_base, uint32_t stream_id, int64_t Nc,
    double* __restrict__ cands, int64_t* __restrict__ datum, uint8_t* __restrict__ domain_err) {
  constexpr int CPB = 256 / SAMPLE_LPC;  // candidates per block
  __shared__ int32_t sdat[CPB];
  __shared__ double srh[HBX_MAX_D];  // 1 / bw per dim
  const int64_t c0 = (int64_t)blockIdx.x * CPB;
  const int nc = (int)(Nc - c0 < CPB ? Nc - c0 : CPB);
  for (int t = threadIdx.x; t < D; t += 256) srh[t] = 1.0 / bw[t];
  if (threadIdx.x < nc) {
    const int64_t i = c0 + threadIdx.x;
    const uint64_t rb = hbx_bits64(draw(seed, counter_base + (uint64_t)i, DATUM_WORD, stream_id), 0);
    const int32_t idx = (int32_t)__umul64hi(rb, (uint64_t)n);  // floor(u * n), u = rb / 2^64
    sdat[threadIdx.x] = idx;
    if (datum) datum[i] = idx;
  }
  __syncthreads();
  const int cl = threadIdx.x / SAMPLE_LPC, g = threadIdx.x % SAMPLE_LPC;
  if (cl >= nc) return;
  const int64_t i = c0 + cl;
  const int32_t idx = sdat[cl];
  const double* xr = X + rows[idx] * (int64_t)D;
  double* out = cands + i * (int64_t)D;
  const int D2 = (D + 1) >> 1;
  bool derr = false;
  HbxU32x4 r;
  for (int k = g; k < D2; k += SAMPLE_LPC) {
    const int q = (k - g) / SAMPLE_LPC;  // this lane's q-th pair: a new block every second pair
    if ((q & 1) == 0) r = draw(seed, counter_base + (uint64_t)i, (uint32_t)(g + SAMPLE_LPC * (q >> 1)), stream_id);
    const uint32_t w0 = (q & 1) ? r.x[2] : r.x[0], w1 = (q & 1) ? r.x[3] : r.x[1];
    const int d = 2 * k;
    const double v0 = sample_dim<TAB>(xr, d, idx, D, bw, srh, levels, tab, bw_factor, w0, &derr);
    if (d + 1 < D) {
      const double v1 = sample_dim<TAB>(xr, d + 1, idx, D, bw, srh, levels, tab, bw_factor, w1, &derr);
      if ((D & 1) == 0) {
        *(double2*)(out + d) = make_double2(v0, v1);
      } else {
        out[d] = v0;
        out[d + 1] = v1;
      }
    } else {
      out[d] = v0;
    }
  }
  if (derr && domain_err) domain_err[i] = 1;  // any of the candidate's lanes (same byte, same value)
}

// The grouped sampler (hbx_kde_sample_groups): kde_sample_pair_kernel<false> per group b of a batched refit
// (hbx_kde_fit's arrays as they lie on the device) -- X base X + seg_off[b] D, rows = order + seg_off[b] (the good
// KDE: the head n_good[b] of the argsort), bw = bw_good + b D -- with candidate (b, i) on the Philox counter
// counter_base + b C + i: the same draw, sample_dim and stores, so its bytes are hbx_kde_sample's for that group
// at counter_base + b C.  Blocks: B x ceil(C / CPB), linear in blockIdx.x.  Groups without a model (n_good[b] <= 0
// or past the segment, hbx_kde_fit's rule) get NaN rows.
//
// MASK (hbx_kde_sample_groups_m): the pool is S requests of Cr candidates (C = S Cr) and want[b][s] says which
// requests are drawn.  The grid is the dense one; a block whose candidates all belong to unwanted requests returns
// before it reads the model, and in a mixed block the lanes of unwanted requests neither draw nor store -- so a wanted
// candidate's bytes are the dense call's, and an unwanted request's rows and error bytes are not written.  The
// <false> instance is the kernel hbx_kde_sample_groups has always launched.
template <bool MASK>
__global__ __launch_bounds__(256) void kde_sample_groups_kernel(
    const double* __restrict__ X, int32_t D, const int64_t* __restrict__ seg_off, const int64_t* __restrict__ order,
    const int64_t* __restrict__ n_good, const double* __restrict__ bw_good, const int32_t* __restrict__ levels,
    double bw_factor, uint64_t seed, uint64_t counter_base, uint32_t stream_id, int64_t C, int32_t tiles,
    double* __restrict__ cands, uint8_t* __restrict__ domain_err, int32_t S, int32_t Cr,
    const uint8_t* __restrict__ want) {
  constexpr int CPB = 256 / SAMPLE_LPC;  // candidates per block
  __shared__ int32_t sdat[CPB];
  __shared__ double srh[HBX_MAX_D];  // 1 / bw per dim
  const int64_t b = (int64_t)blockIdx.x / tiles;
  const int64_t c0 = ((int64_t)blockIdx.x - b * tiles) * CPB;
  const int nc = (int)(C - c0 < CPB ? C - c0 : CPB);
  bool wdraw = true, wlane = true;  // the datum draw of candidate c0 + threadIdx.x, the dims of candidate c0 + cl
  if constexpr (MASK) {
    const uint8_t* wb = want + b * S;
    wdraw = (int)threadIdx.x < nc && wb[(uint32_t)(c0 + threadIdx.x) / (uint32_t)Cr] != 0;
    if (!__syncthreads_or(wdraw)) return;  // (uniform) nothing wanted here: the model is not read
    const int clm = threadIdx.x / SAMPLE_LPC;
    wlane = clm < nc && wb[(uint32_t)(c0 + clm) / (uint32_t)Cr] != 0;
  }
  const int64_t s0 = seg_off[b], n = n_good[b];
  const bool model = n > 0 && n <= seg_off[b + 1] - s0;  // (uniform)
  const int cl = threadIdx.x / SAMPLE_LPC, g = threadIdx.x % SAMPLE_LPC;
  const int D2 = (D + 1) >> 1;
  if (!model) {
    if (cl < nc && wlane) {
      double* out = cands + (b * C + c0 + cl) * (int64_t)D;
      for (int d = g; d < D; d += SAMPLE_LPC) out[d] = NAN;
    }
    return;
  }
  const double* bw = bw_good + b * (int64_t)D;
  const int64_t* rows = order + s0;
  const double* Xs = X + s0 * (int64_t)D;
  for (int t = threadIdx.x; t < D; t += 256) srh[t] = 1.0 / bw[t];
  if (threadIdx.x < nc && wdraw) {
    const uint64_t ctr = counter_base + (uint64_t)(b * C + c0 + threadIdx.x);
    const uint64_t rb = hbx_bits64(draw(seed, ctr, DATUM_WORD, stream_id), 0);
    sdat[threadIdx.x] = (int32_t)__umul64hi(rb, (uint64_t)n);  // floor(u * n), u = rb / 2^64
  }
  __syncthreads();
  if (cl >= nc || !wlane) return;
  const int64_t i = b * C + c0 + cl;  // the candidate's row in cands and its byte in domain_err
  const uint64_t ctr = counter_base + (uint64_t)i;
  const int32_t idx = sdat[cl];
  const double* xr = Xs + rows[idx] * (int64_t)D;
  double* out = cands + i * (int64_t)D;
  bool derr = false;
  HbxU32x4 r;
  for (int k = g; k < D2; k += SAMPLE_LPC) {
    const int q = (k - g) / SAMPLE_LPC;  // this lane's q-th pair: a new block every second pair
    if ((q & 1) == 0) r = draw(seed, ctr, (uint32_t)(g + SAMPLE_LPC * (q >> 1)), stream_id);
    const uint32_t w0 = (q & 1) ? r.x[2] : r.x[0], w1 = (q & 1) ? r.x[3] : r.x[1];
    const int d = 2 * k;
    const double v0 = sample_dim<false>(xr, d, idx, D, bw, srh, levels, nullptr, bw_factor, w0, &derr);
    if (d + 1 < D) {
      const double v1 = sample_dim<false>(xr, d + 1, idx, D, bw, srh, levels, nullptr, bw_factor, w1, &derr);
      if ((D & 1) == 0) {
        *(double2*)(out + d) = make_double2(v0, v1);
      } else {
        out[d] = v0;
        out[d + 1] = v1;
      }
    } else {
      out[d] = v0;
    }
  }
  if (derr && domain_err) domain_err[i] = 1;  // any of the candidate's lanes (same byte, same value)
}

extern "C" {

int hbx_kde_sample_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const double* bw_good, const int32_t* levels, double bw_factor,
                          uint64_t seed, uint64_t counter_base, uint32_t stream_id, int64_t C, double* cands,
                          uint8_t* domain_err, void* stream) {
  if (B < 0 || C < 0 || D < 1 || D > HBX_MAX_D)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_groups: B=%lld C=%lld D=%d", (long long)B, (long long)C, D);
  if (B > INT32_MAX || (C > 0 && B > (int64_t)INT32_MAX / C))
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_groups: B * C = %lld * %lld exceeds int32", (long long)B, (long long)C);
  if (B == 0 || C == 0) return HBX_OK;
  if (!X || !seg_off || !order || !n_good || !bw_good || !levels || !cands)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_groups: null pointer");
  if ((D & 1) == 0 && ((uintptr_t)cands & 15))
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_groups: cands not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (domain_err) HBX_HIP(hipMemsetAsync(domain_err, 0, (size_t)(B * C), s));
  constexpr int CPB = 256 / SAMPLE_LPC;
  const int64_t tiles = (C + CPB - 1) / CPB;
  hipLaunchKernelGGL(kde_sample_groups_kernel<false>, dim3((unsigned)(B * tiles)), dim3(256), 0, s, X, D, seg_off, order,
                     n_good, bw_good, levels, bw_factor, seed, counter_base, stream_id, C, (int32_t)tiles, cands,
                     domain_err, 1, 1, (const uint8_t*)nullptr);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int hbx_kde_sample_groups_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                            const int64_t* n_good, const double* bw_good, const int32_t* levels, double bw_factor,
                            uint64_t seed, uint64_t counter_base, uint32_t stream_id, int64_t S, int64_t C,
                            const uint8_t* want, double* cands, uint8_t* domain_err, void* stream) {
  const char* who = "hbx_kde_sample_groups_m";
  if (B < 0 || S < 0 || C < 0 || D < 1 || D > HBX_MAX_D)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld S=%lld C=%lld D=%d", who, (long long)B, (long long)S, (long long)C, D);
  if (B > INT32_MAX || S > INT32_MAX || (S > 0 && B > (int64_t)INT32_MAX / S) ||
      (C > 0 && B * S > (int64_t)INT32_MAX / C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * S * C = %lld * %lld * %lld exceeds int32", who, (long long)B, (long long)S,
                    (long long)C);
  if (!want)  // every request wanted: the dense call itself
    return hbx_kde_sample_groups(X, D, seg_off, B, order, n_good, bw_good, levels, bw_factor, seed, counter_base,
                                 stream_id, S * C, cands, domain_err, stream);
  if (B == 0 || S == 0 || C == 0) return HBX_OK;
  if (!X || !seg_off || !order || !n_good || !bw_good || !levels || !cands)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if ((D & 1) == 0 && ((uintptr_t)cands & 15)) return hbx_fail(HBX_ERR_ARG, "%s: cands not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = S * C;
  if (domain_err) HBX_HIP(hipMemsetAsync(domain_err, 0, (size_t)(B * P), s));
  constexpr int CPB = 256 / SAMPLE_LPC;
  const int64_t tiles = (P + CPB - 1) / CPB;
  hipLaunchKernelGGL(kde_sample_groups_kernel<true>, dim3((unsigned)(B * tiles)), dim3(256), 0, s, X, D, seg_off, order,
                     n_good, bw_good, levels, bw_factor, seed, counter_base, stream_id, P, (int32_t)tiles, cands,
                     domain_err, (int32_t)S, (int32_t)C, want);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int hbx_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  if (!counter || !key || !out) return hbx_fail(HBX_ERR_ARG, "hbx_philox4x32_10: null pointer");
  HbxU32x4 c;
  for (int k = 0; k < 4; ++k) c.x[k] = counter[k];
  const HbxU32x4 r = hbx_philox4x32_10_impl(c, key[0], key[1]);
  for (int k = 0; k < 4; ++k) out[k] = r.x[k];
  return HBX_OK;
}

int hbx_norm_ppf(const double* p, int64_t n, double* z, void* stream) {
  if (n < 0 || (n > 0 && (!p || !z))) return hbx_fail(HBX_ERR_ARG, "hbx_norm_ppf: bad arguments");
  if (n == 0) return HBX_OK;
  hipLaunchKernelGGL(norm_ppf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, n, z);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int64_t hbx_kde_sample_table_bytes(int64_t n, int32_t D) { return n * (int64_t)D * 16; }

int hbx_kde_sample_table(const double* X, int32_t D, const int64_t* rows, int64_t n, const double* bw,
                         const int32_t* levels, double* tab, void* stream) {
  if (n < 1 || D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_table: n=%lld D=%d", (long long)n, D);
  if (!X || !rows || !bw || !levels || !tab) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample_table: null pointer");
  const int64_t blocks = (n * (int64_t)D + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK;
  hipLaunchKernelGGL(kde_sample_table_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(SAMPLE_BLOCK),
                     0, (hipStream_t)stream, X, D, rows, n, bw, levels, (double2*)tab);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int hbx_kde_sample(const double* X, int32_t D, const int64_t* rows, int64_t n, const double* bw,
                   const int32_t* levels, const double* tab, double bw_factor, uint64_t seed, uint64_t counter_base,
                   uint32_t stream_id, int64_t Nc, double* cands, int64_t* datum, uint8_t* domain_err, void* stream) {
  if (Nc < 0 || D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample: Nc=%lld D=%d", (long long)Nc, D);
  if (Nc == 0) return HBX_OK;
  if (!X || !rows || !bw || !levels || !cands) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample: null pointer");
  if (n < 1 || n > INT32_MAX) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample: n=%lld observations", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (domain_err) HBX_HIP(hipMemsetAsync(domain_err, 0, (size_t)Nc, s));
  if ((D & 1) == 0 && ((uintptr_t)cands & 15)) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample: cands not 16-byte aligned");
  constexpr int CPB = 256 / SAMPLE_LPC;
  const int64_t pb = (Nc + CPB - 1) / CPB;  // one (candidate, pair of dims) per lane
  if (pb > INT32_MAX) return hbx_fail(HBX_ERR_ARG, "hbx_kde_sample: Nc=%lld", (long long)Nc);
  hipLaunchKernelGGL(tab ? kde_sample_pair_kernel<true> : kde_sample_pair_kernel<false>, dim3((unsigned)pb), dim3(256),
                     0, s, X, D, rows, n, bw, levels, (const double2*)tab, bw_factor, seed, counter_base, stream_id,
                     Nc, cands, datum, domain_err);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

}  // extern "C"
