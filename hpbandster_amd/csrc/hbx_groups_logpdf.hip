// hbx_groups_logpdf.hip -- grouped ln-pdf: both KDEs' log densities for every bracket's pool in one call
// (hbx_kde_logpdf_groups; KDEMultivariate.pdf, SM:kernel_density.py:162-196 -> SM:kernels.py:23-65,108-125, per
// bracket after the batched refit bohb.py:220-246).  The grouped form of hbx_kde_logpdf_rtol's contract: every value
// within rtol * max(1, |ln p|) of the reference's ln pdf, -inf where the pdf is 0, NaN where it is NaN or negative.
//
// Inputs are hbx_kde_fit's, as they lie on the device (hbx_groups.hip's header has the layout): no KdeParams, no
// table, no prepare, no host synchronisation.  cand is f64[B][C][D]; ln_l / ln_g are f64[B][C] (either nullable).
//
// Launches, all on the caller's stream:
//   (memset)             the workspace header (the four counters) and the per-(group, KDE) list counts
//   glp_status_kernel    one wave per group: status[b] = HBX_ACQ_NO_MODEL / HBX_ACQ_UNSUPPORTED (hbx_kde_acquire_groups'
//                        rules) and, per KDE, HBX_GRP_EXACT_L / _G; the later kernels read status[b]
//   glp_dd_kernel        (not with HBX_LOGPDF_FP64_ONLY) the fp32 pass: writes what its bound certifies, lists the rest
//   glp_f64_kernel       the fp64 log-space pass over the listed candidates (FP64_ONLY: over all); also the NaN fill
//                        of groups without a usable model
//   glp_exact_kernel     KDEs with an EXACT bit: ln of the bit-exact fp64 pdf (hbx_exact_impl.h, the single path's
//                        functions fed a per-group parameter view), every candidate
// Grids are (B x ceil(C / 64), KDEs requested): a block is one 64-candidate tile of one group and one KDE.
// Correctness never rests on the fp32 pass: it only decides which values the fp64 pass need not compute.
//
// A KDE is EXACT when a categorical match factor is negative (h > 1), a categorical dim has a single observed level
// (c == 1, h == 0), a bandwidth is not a positive finite number, or the dims exceed the slot bucket picked from D
// (hbx_groups.hip's buckets: D <= 8, 16, 32 any mix; D <= 96 up to 64 continuous + 32 categorical).  Its values are
// ln of the reference's own fp64 pdf: NaN where that is negative or NaN, -inf where it underflows to 0.
//
// The fp32 pass, glp_dd_kernel<DCP, DUP, NW, DT>: groups_screen_kernel's structure for one KDE -- lane = candidate
// (its scaled coordinates in registers), the block's NW waves take the KDE's 64-observation chunks in turn, each
// gathered through `order`, centred, scaled and staged as fp32 in the wave's LDS rows, read back as broadcasts.  Per
// pair, in log2 units, direct differences (no expansion, so no cancellation):
//     t_ij = sum_c -(a_ic - b_jc)^2 + sum_u m_iju delta_u,      a = fl(s_c (x_c - mu_c)), b = fl(s_c (X_jc - mu_c))
//   s_c = sqrt(log2 e / 2) / h_c, mu_c = mean of the group's first <= 64 good rows, m = [x_u == X_ju], delta_u =
//   log2(1 - h_u) - log2(h_u / (c_u - 1)) (-1e30 where 1 - h_u == 0: the term is exactly 0).  The constant part
//   lb = sum_u log2(h_u / (c_u - 1)) stays out of the chain and is added in fp64 at the end.
//   The sum is kde_logpdf_dd_kernel's (hbx_logpdf.hip): terms 2^(t - m) against an integer reference point m = the
//   running max ceil(t) (a new maximum rescales both sums by an exact ldexp), GLP_G = 4 terms summed in fp32, the
//   groups accumulated in fp64; the waves' (m, S) merge by ldexp in fp64.
//
//   The bound (u = 2^-24, K = 40), per candidate i, with R_c = |a_ic| + max_j |b_jc| (the maxima taken while
//   staging), sdp = sum_u max(delta_u, 0), sad = sum_u |delta_u| over the finite deltas, M the final reference point,
//   n the KDE's rows, L = the chain's fma steps + 1:
//     coordinates  a and b are fp64 products rounded once, dd = fl(a - b): |dd_c - d*_c| <= e_c = 2.02 u R_c, so
//                  sum_c |dd_c^2 - d*_c^2| <= 2 sqrt(q*) |e| + |e|^2 (Cauchy-Schwarz), q* = sum_c d*_c^2 the pair's true
//                  squared distance, |e|^2 = (2.02 u)^2 sum_c R_c^2.
//     the chain    L roundings of at most u |partial|, |partial| <= sad + q~ (q~ the computed distance), and u sad for
//                  the deltas' own rounding to fp32; the match m is exact (integer codes below 2^24).
//     => for a pair with q* <= Q:  |t - t*| <= E(Q) = 2 sqrt(Q) |e| + |e|^2 + L u (sad + Q + 2 sqrt(Q) |e| + |e|^2)
//                  + u sad + 2^-48 Q (the fp64 roundings of s_c and of the products).
//     which pairs  Q = max(0, sdp - (M - 1)) + K + 2, and E(Q) <= 1/2 is required below.  The pair that set M has
//                  t > M - 1, hence q~ < sdp - (M - 1) + L u (sad + q~); q - 2 sqrt(q) |e| - |e|^2 grows with q and at
//                  q = Q - K - 1 exceeds that (by 1/2 - E(Q) >= 0), so q* < Q - K - 1, its own error is within E(Q) and
//                  its true exponent is >= M - 1.5: so is the largest true exponent t*max.  Past Q, E grows by
//                  |e| / sqrt(q) + 1.01 L u <= E(Q) / (2 Q) + 1.01 L u < 1/128 per unit of q (Q >= 42).  A pair with
//                  q* > Q therefore has t* <= sdp* - q* < t*max - K - 1 and a computed exponent t <= sdp* - q* + E(Q)
//                  + (q* - Q) / 128 <= sdp* - Q + 1/2 < M - K - 2: true and computed, such pairs weigh less than
//                  2 n 2^-K of the sum (>= 1/2 in units of 2^M; the 2 of Q absorbs sdp* - sdp).  The clamped rescale
//                  (a maximum rising by more than 250) and fp32 flushes below 2^-126 are far inside the other 2 n 2^-K.
//     the terms    the exponent t - m is rounded once: (K + 3) u for the pairs that count (the rest: 0.7 u |x| 2^-|x| <
//                  2^-K each); v_exp_f32 is within 2 ulp = 2^-22; a group's fp32 sum (GLP_G - 1) u; the fp64
//                  accumulation and merge (n + NW) 2^-52.
//     => Et = E(Q) + (K + 3) u,  rel = 2^Et - 1 + 2^-22 + (GLP_G - 1) u + (n + NW) 2^-52 + 4 n 2^-K,
//        |ln p_est - ln p| <= rel / (1 - rel) + 2^-48 (|ln S| + |lb ln 2| + |norm| + |ln p|)      (the fp64 epilogue)
//   A value is written when Et < 1/2, rel < 1/2, every input and sum is finite, S > 0 and the bound is within
//   0.99 rtol max(1, |ln p_est|); every other candidate goes to the (group, KDE)'s own list segment of C entries, so a
//   list cannot overflow.  The bound is evaluated in fp64 (its own rounding is 2^-50 of itself, inside the 0.99).
//
// The fp64 pass, glp_f64_kernel<DCP, DUP, NW, EXP64>: kde_logpdf_tiled_kernel's evaluation (hbx_logpdf.hip: direct
// differences -((x - X) / (h sqrt 2))^2, ln(1 - h) or ln(h / (c - 1)) per categorical dim, a running log-sum-exp with
// fp64 sums, 2^(t' - m') by v_exp_f32 on the fp32-rounded exponent: |ln S_est - ln S| < 4e-6, its header has the
// argument; EXP64 -- fp64 exp2 -- for rtol < 1e-5), fed the per-group view, lane = listed candidate, the waves
// splitting the KDE's 32-row chunks as in the fp32 pass and merging their (m, S) with fp64 exp2.  Categorical codes
// are compared as fp32 (cand_code): exact for observed codes (integers in [0, 1024)), and a candidate value that is
// no such integer matches nothing, in the reference as here.
#include <math.h>

#include "hbx_exact_impl.h"

#define GLP_HEAD 256  // workspace header: the four counters (u64) in its first 32 bytes
#define GLP_G 4       // terms per fp32 group
#define GLP_K 40      // pairs more than K log2 units under the largest are bounded, not tracked
#define GLP_BAD (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED)

struct GlpArgs {
  const double* X;
  const int64_t* seg_off;
  const int64_t* order;
  const int64_t* n_good;
  const int64_t* n_bad;
  const int32_t* vartype;
  const double* bw_good;
  const double* bw_bad;
  const int32_t* nlev_good;
  const int32_t* nlev_bad;
  const double* cand;
  int64_t B, C;
  int32_t D, tiles;  // tiles = ceil(C / 64)
  int32_t dcp, dup;  // the slot bucket (from D alone)
  int32_t kd0;       // first KDE of the launch's grid.y (0: good / ln_l, 1: bad / ln_g)
  int32_t fp64_only;
  double rtol;
  double* out[2];    // ln_l, ln_g (nullable)
  int32_t* status;
  unsigned long long* stat;  // the header's counters
  int32_t* cnt;              // [B][2] listed candidates per (group, KDE)
  int32_t* list;             // [B][2][C]
};

// the per-group parameter view the exact functions read (hbx_exact_impl.h)
struct GlpView {
  int32_t n;
  const double* bw;
  const int32_t* vartype;
  const int32_t* nlev;
  double prod_bw_c;
};

// status[b]: hbx_kde_fit's skip rule and hbx_kde_prepare's per-dim rules as hbx_kde_acquire_groups applies them
// (grp_status, hbx_groups.hip), with the exact-only conditions kept per KDE.  One wave per group.
__global__ __launch_bounds__(256) void glp_status_kernel(GlpArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= A.B) return;  // whole wave
  const int64_t n = A.seg_off[b + 1] - A.seg_off[b], ng = A.n_good[b], nb = A.n_bad[b];
  if (ng <= 0 || ng > n || nb <= 0 || nb > n) {
    if (lane == 0) A.status[b] = HBX_ACQ_NO_MODEL;
    return;
  }
  int st = 0, dc = 0, du = 0;
  for (int d0 = 0; d0 < A.D; d0 += 64) {
    const int d = d0 + lane;
    const bool live = d < A.D;
    const bool cont = live && A.vartype[d] == 0;
    dc += __popcll(__ballot(cont));
    du += __popcll(__ballot(live && !cont));
    if (!live) continue;
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {
      const int ex = kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L;
      const double h = (kd ? A.bw_bad : A.bw_good)[b * A.D + d];
      if (cont) {
        if (!(h > 0.0 && h < INFINITY)) st |= ex;  // pdf NaN (or 0) everywhere: the exact path says which
      } else {
        const int c = (kd ? A.nlev_bad : A.nlev_good)[b * A.D + d];
        if (c == 1 && h == 0.0)
          st |= ex;  // one observed level: match -> 1, mismatch -> 0 / 0
        else if (c < 2 || !(h > 0.0) || h != h)
          st |= HBX_ACQ_UNSUPPORTED;  // (c == -1: codes not integers in [0, 1024))
        else if (!(h < INFINITY) || 1.0 - h < 0.0)
          st |= ex;  // (h > 1: a negative match factor, signed sums)
      }
    }
  }
  st = (int)wave_reduce_dpp((uint32_t)st, OpOr());
  if (dc > A.dcp || du > A.dup) st |= HBX_GRP_EXACT_L | HBX_GRP_EXACT_G;
  if (st & HBX_ACQ_UNSUPPORTED) st = HBX_ACQ_UNSUPPORTED;
  if (lane == 0) A.status[b] = st;
}

// The dims of a usable KDE sorted into slots in dim order by one wave: continuous dims to cdim[0 .. dc), categorical
// dims to udim[0 .. du); every lane returns the counts (dc <= DCP, du <= DUP: the status kernel checked the bucket).
__device__ __forceinline__ void glp_slots(const GlpArgs& A, int lane, int32_t* cdim, int32_t* udim, int* dc, int* du) {
  int kc = 0, ku = 0;
  for (int d0 = 0; d0 < A.D; d0 += 64) {
    const int d = d0 + lane;
    const bool cont = d < A.D && A.vartype[d] == 0, cat = d < A.D && !cont;
    const uint64_t mc = __ballot(cont), mu = __ballot(cat), below = (1ull << lane) - 1ull;
    if (cont) cdim[kc + __popcll(mc & below)] = d;
    if (cat) udim[ku + __popcll(mu & below)] = d;
    kc += __popcll(mc);
    ku += __popcll(mu);
  }
  *dc = kc;
  *du = ku;
}

// One staged chunk's pairs for this lane's candidate: rows[0 .. jmax) of the wave's LDS rows (stride rs floats:
// continuous slots from 0, categorical slots from 4 dcq), GLP_G terms per fp32 group, the groups into S.
// QC >= 0: QC continuous and QU categorical 4-slot pieces at compile time (every LDS read of a row issued before its
// first use, grp_pairs_fast's reason); QC < 0: dcq / duq pieces with a uniform branch each.
template <int DCP, int DUP, int QC, int QU>
__device__ __forceinline__ void glp_pairs(const float* __restrict__ rows, int rs, int jmax, int dcq, int duq,
                                          const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                          float& m, double& S) {
  for (int j0 = 0; j0 < jmax; j0 += GLP_G) {
    float s4 = 0.f;
#pragma unroll
    for (int g = 0; g < GLP_G; ++g) {
      if (j0 + g >= jmax) break;  // uniform
      const float4* rj = (const float4*)(rows + (j0 + g) * rs);
      float t = 0.f;
      if constexpr (QC >= 0) {
        static_assert(4 * QC <= DCP && 4 * QU <= DUP, "pieces within the slots");
        float4 vc[QC > 0 ? QC : 1], vu[QU > 0 ? QU : 1];
#pragma unroll
        for (int q = 0; q < QC; ++q) vc[q] = rj[q];
#pragma unroll
        for (int q = 0; q < QU; ++q) vu[q] = rj[QC + q];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
          const float4 v = vc[q];
          const float d0 = xc[4 * q] - v.x, d1 = xc[4 * q + 1] - v.y, d2 = xc[4 * q + 2] - v.z, d3 = xc[4 * q + 3] - v.w;
          t = fmaf(-d0, d0, t);
          t = fmaf(-d1, d1, t);
          t = fmaf(-d2, d2, t);
          t = fmaf(-d3, d3, t);
        }
#pragma unroll
        for (int q = 0; q < QU; ++q) {
          const float4 v = vu[q];
          t = fmaf(cat_match(xu[4 * q], v.x), dl[4 * q], t);
          t = fmaf(cat_match(xu[4 * q + 1], v.y), dl[4 * q + 1], t);
          t = fmaf(cat_match(xu[4 * q + 2], v.z), dl[4 * q + 2], t);
          t = fmaf(cat_match(xu[4 * q + 3], v.w), dl[4 * q + 3], t);
        }
      } else {
#pragma unroll
        for (int q = 0; q < DCP / 4; ++q)
          if (q < dcq) {  // uniform
            const float4 v = rj[q];
            const float d0 = xc[4 * q] - v.x, d1 = xc[4 * q + 1] - v.y, d2 = xc[4 * q + 2] - v.z, d3 = xc[4 * q + 3] - v.w;
            t = fmaf(-d0, d0, t);
            t = fmaf(-d1, d1, t);
            t = fmaf(-d2, d2, t);
            t = fmaf(-d3, d3, t);
          }
#pragma unroll
        for (int q = 0; q < DUP / 4; ++q)
          if (q < duq) {  // uniform
            const float4 v = rj[dcq + q];
            t = fmaf(cat_match(xu[4 * q], v.x), dl[4 * q], t);
            t = fmaf(cat_match(xu[4 * q + 1], v.y), dl[4 * q + 1], t);
            t = fmaf(cat_match(xu[4 * q + 2], v.z), dl[4 * q + 2], t);
            t = fmaf(cat_match(xu[4 * q + 3], v.w), dl[4 * q + 3], t);
          }
      }
      const float tc = ceilf(t);
      if (tc > m) {  // a new reference point (integer): exact rescale of both sums
        const int sh = (int)fmaxf(m - tc, -250.f);
        s4 = ldexpf(s4, sh);
        S = ldexp(S, sh);
        m = tc;
      }
      s4 += __builtin_amdgcn_exp2f(t - m);
    }
    S += (double)s4;
  }
}

template <int DCP, int DUP, int NW, int DT>
__global__ __launch_bounds__(64 * NW) void glp_dd_kernel(GlpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  __shared__ double s_scale[DCP], s_mu[DCP];
  __shared__ float s_delta[DUP];
  __shared__ int32_t s_cdim[DCP], s_udim[DUP];
  __shared__ uint32_t s_bmax[DCP];
  __shared__ int32_t s_doff[DCP + DUP];                // dim -> float offset of its slot in a staged row
  __shared__ double s_dsc[DCP + DUP], s_dmu[DCP + DUP];  // dim -> scale (categorical: 1) and centre (0)
  __shared__ float s_pm[NW][64];
  __shared__ double s_ps[NW][64];
  __shared__ int32_t s_i[2];
  __shared__ double s_norm, s_lbln, s_sdp, s_sad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  if (st & (GLP_BAD | (kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L))) return;  // uniform: the later kernels write these
  const int64_t i = (int64_t)tile * 64 + lane;
  const bool valid = i < A.C;
  if (wave == 0) {
    int dc, du;
    glp_slots(A, lane, s_cdim, s_udim, &dc, &du);
    if (lane == 0) {
      s_i[0] = dc;
      s_i[1] = du;
    }
  }
  __syncthreads();
  const int dc = s_i[0], du = s_i[1];
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t ng = A.n_good[b], nk = kd ? A.n_bad[b] : ng;
  const double* Xs = A.X + s0 * D;
  const int64_t* ord = A.order + s0;
  const int64_t* rows = ord + (kd ? n - nk : 0);
  const double* bw = (kd ? A.bw_bad : A.bw_good) + b * D;
  const int32_t* nlev = (kd ? A.nlev_bad : A.nlev_good) + b * D;
  // the row layout: continuous slots from 0, categorical slots from 4 dcq.  Compile-time piece counts serve dc <= 32
  // in 2 / 4 / 6 / 8 pieces with du <= 8 in 0 / 2 pieces (config #5's 24c + 8u: 6 + 2); the rest the exact counts
  const int qcs = dc <= 8 ? 2 : dc <= 16 ? 4 : dc <= 24 ? 6 : 8;
  const bool fast = dc <= 32 && du <= 8 && 4 * qcs <= DCP && DUP >= 8;
  const int dcq = fast ? qcs : (dc + 3) >> 2;
  const int duq = fast ? (du ? 2 : 0) : (du + 3) >> 2;
  const int dc4 = 4 * dcq, du4 = 4 * duq;
  const int rs = dc4 + du4 + 4;  // <= DT + 4
  const int rpp = D <= 64 ? 64 / D : 1;  // rows per staging pass
  for (int e = tid; e < NT * rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  for (int k = tid; k < DCP; k += NT) {
    s_bmax[k] = 0u;
    if (k < dc) {
      const int d = s_cdim[k];
      const int nm = (int)(ng < 64 ? ng : 64);
      double sum = 0.0;
#pragma unroll 16
      for (int j = 0; j < nm; ++j) sum += Xs[ord[j] * D + d];
      double mu = sum / (double)nm;
      if (!(mu - mu == 0.0)) mu = 0.0;
      s_mu[k] = mu;
      s_dmu[d] = mu;
      s_doff[d] = k;
      s_scale[k] = sqrt(M_LOG2E / 2.0) / bw[d];
      s_dsc[d] = s_scale[k];
    } else {
      s_mu[k] = 0.0;
      s_scale[k] = 0.0;
    }
  }
  for (int u = tid; u < DUP; u += NT) {
    float dl = 0.f;
    if (u < du) {
      const int d = s_udim[u];
      s_doff[d] = dc4 + u;
      s_dsc[d] = 1.0;
      s_dmu[d] = 0.0;
      const double h = bw[d], a = 1.0 - h;  // (a >= 0: a negative factor is an EXACT KDE)
      dl = (a == 0.0) ? -1e30f : (float)(log2(a) - log2(h / (double)(nlev[d] - 1)));
    }
    s_delta[u] = dl;
  }
  __syncthreads();
  if (tid == 0) {  // the sums in slot order (deterministic)
    double sl = 0.0, lbln = 0.0, sdp = 0.0, sad = 0.0;
    for (int k = 0; k < dc; ++k) sl += log(bw[s_cdim[k]]);
    for (int u = 0; u < du; ++u) {
      const int d = s_udim[u];
      lbln += log(bw[d] / (double)(nlev[d] - 1));
      if (s_delta[u] > -1e29f) {
        sdp += fmax((double)s_delta[u], 0.0);
        sad += fabs((double)s_delta[u]);
      }
    }
    s_norm = -log((double)nk) - sl - 0.5 * (double)dc * log(2.0 * M_PI);
    s_lbln = lbln;
    s_sdp = sdp;
    s_sad = sad;
  }
  __syncthreads();
  const double* x = A.cand + (b * A.C + (valid ? i : (int64_t)tile * 64)) * D;
  bool certified = true;
  float xc[DCP], xu[DUP], dl[DUP];
#pragma unroll
  for (int k = 0; k < DCP; ++k) {
    xc[k] = 0.f;
    if (k < dc) {
      const double xv = x[s_cdim[k]];
      certified = certified && (xv - xv == 0.0);
      xc[k] = (float)(s_scale[k] * (xv - s_mu[k]));
    }
  }
#pragma unroll
  for (int u = 0; u < DUP; ++u) {
    xu[u] = 0.f;
    if (u < du) {
      const double xv = x[s_udim[u]];
      certified = certified && (xv - xv == 0.0);
      xu[u] = cand_code(xv);
    }
    dl[u] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_delta[u])));
  }
  float m = -INFINITY;
  double S = 0.0;
  float* wrows = sobs + (size_t)wave * 64 * rs;
  for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * 64) {  // uniform trip count: the barriers are block-wide
    __syncthreads();  // (the rows of the previous round are read)
    const int64_t j0 = c0 + (int64_t)wave * 64;
    const int jmax = (int)(nk - j0 < 64 ? (nk - j0 > 0 ? nk - j0 : 0) : 64);
    if (jmax > 0) {
      // lane = (row in pass, dim): a row's D doubles are read by consecutive lanes (coalesced), 16 passes of loads in
      // flight; dims past 64 take further rounds (db).  The chunk's row positions come in one coalesced load and
      // reach the lanes by a lane exchange (groups_screen_kernel's staging).
      const int myrow = (int)rows[j0 + (lane < jmax ? lane : 0)];  // (positions local to the segment: < 2^31)
      for (int db = 0; db < D; db += 64) {
        const int lr = D <= 64 ? lane / D : 0;
        const int ld = db + (D <= 64 ? lane - lr * D : lane);
        const bool act = lr < rpp && ld < D;
        const int off = act ? s_doff[ld] : 0;
        const double sc = act ? s_dsc[ld] : 0.0, mu = act ? s_dmu[ld] : 0.0;
        uint32_t bm = 0u;  // |b| maximum of this lane's dim (non-negative floats order as their bits; NaN above all)
        for (int p0 = 0; p0 < jmax; p0 += 16 * rpp) {
          double t[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int r = p0 + q * rpp + lr;
            const int ri = __shfl(myrow, r < jmax ? r : 0);  // (every lane takes part in the exchange)
            t[q] = (act && r < jmax) ? Xs[(int64_t)ri * D + ld] : 0.0;
          }
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int r = p0 + q * rpp + lr;
            if (act && r < jmax) {
              const float v = (float)(sc * (t[q] - mu));
              wrows[r * rs + off] = v;
              bm = max(bm, __float_as_uint(fabsf(v)));
            }
          }
        }
        if (act && off < dc) atomicMax(&s_bmax[off], bm);
      }
    }
    __syncthreads();
    if (jmax > 0) {
      if (fast && qcs == 2 && du == 0)
        glp_pairs<DCP, DUP, 2, 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && qcs == 2)
        glp_pairs<DCP, DUP, 2, DUP >= 8 ? 2 : 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && qcs == 4 && du == 0)
        glp_pairs<DCP, DUP, DCP >= 16 ? 4 : 0, 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && qcs == 4)
        glp_pairs<DCP, DUP, DCP >= 16 ? 4 : 0, DUP >= 8 ? 2 : 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && qcs == 6 && du == 0)
        glp_pairs<DCP, DUP, DCP >= 24 ? 6 : 0, 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && qcs == 6)
        glp_pairs<DCP, DUP, DCP >= 24 ? 6 : 0, DUP >= 8 ? 2 : 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast && du == 0)
        glp_pairs<DCP, DUP, DCP >= 32 ? 8 : 0, 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else if (fast)
        glp_pairs<DCP, DUP, DCP >= 32 ? 8 : 0, DUP >= 8 ? 2 : 0>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
      else
        glp_pairs<DCP, DUP, -1, -1>(wrows, rs, jmax, dcq, duq, xc, xu, dl, m, S);
    }
  }
  s_pm[wave][lane] = m;
  s_ps[wave][lane] = S;
  __syncthreads();  // (also: every row of the KDE is staged, s_bmax is complete)
  if (wave != 0) return;
  // merge the waves' partials in wave order
  float M = -INFINITY;
  bool bad = false;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float mw = s_pm[w][lane];
    bad = bad || mw != mw;  // (fmaxf drops a NaN)
    M = fmaxf(M, mw);
  }
  double St = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float mw = s_pm[w][lane];
    if (mw > -INFINITY) St += ldexp(s_ps[w][lane], (int)fmaxf(mw - M, -2000.f));
  }
  // the bound (header), in fp64
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < DCP; ++k)
    if (k < dc) {
      const double r = (double)fabsf(xc[k]) + (double)__uint_as_float(s_bmax[k]);
      r2 += r * r;
    }
  const double u24 = 0x1p-24, sad = s_sad;
  const double en = 2.02 * u24 * sqrt(r2) * (1.0 + 0x1p-20);
  const double Q = fmax(0.0, s_sdp - ((double)M - 1.0)) + (double)GLP_K + 2.0;
  const double ein = 2.0 * sqrt(Q) * en + en * en;
  const double L = (double)(dc4 + du4 + 1);
  const double Et = ein + L * u24 * (sad + Q + ein) + u24 * sad + 0x1p-48 * Q + (double)(GLP_K + 3) * u24;
  const double rel = exp2(Et * (1.0 + 0x1p-20)) - 1.0 + 0x1p-22 + (double)(GLP_G - 1) * u24 +
                     (double)(nk + NW) * 0x1p-52 + 4.0 * (double)nk * exp2(-(double)GLP_K);
  const double lnS = log(St) + (double)M * M_LN2;
  const double lp = lnS + s_lbln + s_norm;
  const double bound = rel / (1.0 - rel) + 0x1p-48 * (fabs(lnS) + fabs(s_lbln) + fabs(s_norm) + fabs(lp));
  const bool ok = valid && certified && !bad && St > 0.0 && St - St == 0.0 && M - M == 0.f && lp - lp == 0.0 &&
                  Et < 0.5 && rel < 0.5 && bound <= 0.99 * A.rtol * fmax(1.0, fabs(lp));
  if (ok) A.out[kd][b * A.C + i] = lp;
  const uint64_t okb = __ballot(ok), bal = __ballot(valid && !ok);
  if (bal) {  // one atomic per tile; the segment holds C entries and a candidate is listed once
    const int first = __ffsll((long long)bal) - 1;
    int32_t base = 0;
    if (lane == first) base = atomicAdd(&A.cnt[b * 2 + kd], __popcll(bal));
    base = __shfl(base, first);
    if (valid && !ok) A.list[(b * 2 + kd) * A.C + base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)i;
  }
  if (lane == 0 && okb) atomicAdd(&A.stat[0], (unsigned long long)__popcll(okb));
}

// the fp64 log-space pass (header): tile `tile` of the (group, KDE)'s list -- or, fp64_only, of its pool
template <int DCP, int DUP, int NW, bool EXP64>
__global__ __launch_bounds__(64 * NW) void glp_f64_kernel(GlpArgs A) {
  constexpr int NT = 64 * NW, OB = 32;  // observations per wave and round
  constexpr int RB = DCP * 8 + DUP * 4;  // bytes per staged row: DCP scaled coordinates (f64), DUP codes (f32)
  __shared__ __align__(16) char srow[NW * OB * RB];
  __shared__ double s_sa[DCP], s_dl[DUP];
  __shared__ int32_t s_cdim[DCP], s_udim[DUP];
  __shared__ double s_pm[NW][64], s_ps[NW][64];
  __shared__ int32_t s_pn[NW][64];
  __shared__ int32_t s_i[2];
  __shared__ double s_lconst;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  double* out = A.out[kd] + b * A.C;
  if (st & GLP_BAD) {  // no usable model: every output of the group is NaN
    const int64_t i = (int64_t)tile * 64 + lane;
    if (wave == 0) {
      if (i < A.C) out[i] = NAN;
      const uint64_t bal = __ballot(i < A.C);
      if (lane == 0) atomicAdd(&A.stat[3], (unsigned long long)__popcll(bal));
    }
    return;
  }
  if (st & (kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L)) return;  // glp_exact_kernel
  const int64_t cnt = A.fp64_only ? A.C : (int64_t)A.cnt[b * 2 + kd];
  const int64_t pi = (int64_t)tile * 64 + lane;
  if ((int64_t)tile * 64 >= cnt) return;  // uniform
  const bool valid = pi < cnt;
  const int64_t p = valid ? (A.fp64_only ? pi : (int64_t)A.list[(b * 2 + kd) * A.C + pi]) : 0;
  if (wave == 0) {
    int dc, du;
    glp_slots(A, lane, s_cdim, s_udim, &dc, &du);
    if (lane == 0) {
      s_i[0] = dc;
      s_i[1] = du;
    }
  }
  __syncthreads();
  const int dc = s_i[0], du = s_i[1];
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t nk = kd ? A.n_bad[b] : A.n_good[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* rows = A.order + s0 + (kd ? n - nk : 0);
  const double* bw = (kd ? A.bw_bad : A.bw_good) + b * D;
  const int32_t* nlev = (kd ? A.nlev_bad : A.nlev_good) + b * D;
  // per-slot constants: a_c = 1 / (h sqrt 2); categorical: ln(h / (c - 1)) + [match] (ln(1 - h) - ln(h / (c - 1))),
  // the first part summed into the constant (kde_logpdf_tiled_kernel's)
  for (int k = tid; k < DCP; k += NT) s_sa[k] = k < dc ? 1.0 / (bw[s_cdim[k]] * 1.4142135623730951) : 0.0;
  for (int u = tid; u < DUP; u += NT) {
    double v = 0.0;
    if (u < du) {
      const int d = s_udim[u];
      v = log(1. - bw[d]) - log(bw[d] / (double)(nlev[d] - 1));
    }
    s_dl[u] = v;
  }
  if (tid == 0) {
    double lc = -log((double)nk);
    for (int k = 0; k < dc; ++k) lc -= log(bw[s_cdim[k]]) + 0.91893853320467274178;  // ln(h sqrt(2 pi))
    for (int u = 0; u < du; ++u) {
      const int d = s_udim[u];
      lc += log(bw[d] / (double)(nlev[d] - 1));
    }
    s_lconst = lc;
  }
  __syncthreads();
  const int dcq = (dc + 3) >> 2, duq = (du + 3) >> 2;
  const double* x = A.cand + (b * A.C + p) * D;
  double xc[DCP];
  float xu[DUP];
#pragma unroll
  for (int k = 0; k < DCP; ++k) xc[k] = k < dc ? x[s_cdim[k]] * s_sa[k] : 0.0;
#pragma unroll
  for (int u = 0; u < DUP; ++u) xu[u] = u < du ? cand_code(x[s_udim[u]]) : 0.f;
  char* wrow = srow + (size_t)wave * OB * RB;
  for (int e = lane; e < OB * RB / 4; e += 64) ((float*)wrow)[e] = 0.f;  // (the padding slots stay 0)
  double m = -INFINITY, S = 0.0;
  bool nan = false;
  for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * OB) {  // uniform trip count: the barriers are block-wide
    __syncthreads();  // (the rows of the previous round are read)
    const int64_t j0 = c0 + (int64_t)wave * OB;
    const int jmax = (int)(nk - j0 < OB ? (nk - j0 > 0 ? nk - j0 : 0) : OB);
    for (int e = lane; e < jmax * D; e += 64) {  // a row's slots by consecutive lanes
      const int r = e / D, k = e - r * D;
      const double* xr = Xs + rows[j0 + r] * (int64_t)D;
      if (k < dc)
        ((double*)(wrow + r * RB))[k] = xr[s_cdim[k]] * s_sa[k];
      else
        ((float*)(wrow + r * RB + DCP * 8))[k - dc] = (float)xr[s_udim[k - dc]];  // (an integer in [0, 1024): exact)
    }
    __syncthreads();
    for (int j = 0; j < jmax; ++j) {
      const double2* rc = (const double2*)(wrow + j * RB);
      const float4* ru = (const float4*)(wrow + j * RB + DCP * 8);
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < DCP / 4; ++q)
        if (q < dcq) {  // uniform
          const double2 v0 = rc[2 * q], v1 = rc[2 * q + 1];
          const double d0 = xc[4 * q] - v0.x, d1 = xc[4 * q + 1] - v0.y, d2 = xc[4 * q + 2] - v1.x,
                       d3 = xc[4 * q + 3] - v1.y;
          t = fma(-d0, d0, t);
          t = fma(-d1, d1, t);
          t = fma(-d2, d2, t);
          t = fma(-d3, d3, t);
        }
#pragma unroll
      for (int q = 0; q < DUP / 4; ++q)
        if (q < duq) {  // uniform
          const float4 v = ru[q];
          t += (xu[4 * q] == v.x) ? s_dl[4 * q] : 0.0;
          t += (xu[4 * q + 1] == v.y) ? s_dl[4 * q + 1] : 0.0;
          t += (xu[4 * q + 2] == v.z) ? s_dl[4 * q + 2] : 0.0;
          t += (xu[4 * q + 3] == v.w) ? s_dl[4 * q + 3] : 0.0;
        }
      const double tl = t * 1.4426950408889634;  // log2 units
      if (tl > m) {
        S = (m > -INFINITY ? S * (EXP64 ? exp2(m - tl) : (double)__builtin_amdgcn_exp2f((float)(m - tl))) : 0.0) + 1.0;
        m = tl;
      } else if (tl > -INFINITY) {
        S += EXP64 ? exp2(tl - m) : (double)__builtin_amdgcn_exp2f((float)(tl - m));
      } else if (tl != tl) {
        nan = true;
      }
    }
  }
  s_pm[wave][lane] = m;
  s_ps[wave][lane] = S;
  s_pn[wave][lane] = nan;
  __syncthreads();
  if (wave != 0) return;
  double M = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    M = fmax(M, s_pm[w][lane]);
    nan = nan || s_pn[w][lane];
  }
  double St = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w)
    if (s_pm[w][lane] > -INFINITY) St += s_ps[w][lane] * exp2(s_pm[w][lane] - M);
  if (valid) out[p] = nan ? NAN : (M > -INFINITY ? (M + log2(St)) * 0.69314718055994531 + s_lconst : -INFINITY);
  const uint64_t bal = __ballot(valid);
  if (lane == 0) atomicAdd(&A.stat[1], (unsigned long long)__popcll(bal));
}

// EXACT KDEs: ln of the bit-exact fp64 pdf of every candidate of the tile, each by the whole block
// (groups_select_kernel's use of exact_setup / exact_pdf)
__global__ __launch_bounds__(EXACT_THREADS) void glp_exact_kernel(GlpArgs A) {
  __shared__ ExactShared sh;
  __shared__ GlpView vw;
  const int D = A.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  if ((st & GLP_BAD) || !(st & (kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L))) return;  // uniform
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t nk = kd ? A.n_bad[b] : A.n_good[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* rows = A.order + s0 + (kd ? n - nk : 0);
  if (threadIdx.x == 0) {  // prod(bw[iscontinuous]) sequentially in dim order: the reference's order
    GlpView v;
    v.n = (int32_t)nk;
    v.bw = (kd ? A.bw_bad : A.bw_good) + b * D;
    v.nlev = (kd ? A.nlev_bad : A.nlev_good) + b * D;
    v.vartype = A.vartype;
    double p = 1.0;
    for (int d = 0; d < D; ++d) p *= (A.vartype[d] == 0) ? v.bw[d] : 1.0;
    v.prod_bw_c = p;
    vw = v;
  }
  __syncthreads();
  const int64_t i0 = (int64_t)tile * 64, i1 = i0 + 64 < A.C ? i0 + 64 : A.C;
  for (int64_t i = i0; i < i1; ++i) {
    exact_setup(&vw, D, A.cand + (b * A.C + i) * D, &sh);
    const double v = exact_pdf(Xs, D, rows, &vw, &sh);
    if (threadIdx.x == 0) A.out[kd][b * A.C + i] = log(v);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(&A.stat[2], (unsigned long long)(i1 - i0));
}

// B * C within int32 (what every grid, list entry and count relies on)
static bool glp_counts_ok(int64_t B, int64_t C) {
  if (B < 0 || C < 0 || B > INT32_MAX) return false;
  return !(C > 0 && B > (int64_t)INT32_MAX / C);
}

static int64_t glp_cnt_bytes(int64_t B) { return (B * 2 * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15; }

template <bool E64>
static void glp_launch_f64(const GlpArgs& A, dim3 grid, hipStream_t s) {
  if (A.D <= 8)
    hipLaunchKernelGGL((glp_f64_kernel<8, 8, 4, E64>), grid, dim3(256), 0, s, A);
  else if (A.D <= 16)
    hipLaunchKernelGGL((glp_f64_kernel<16, 16, 4, E64>), grid, dim3(256), 0, s, A);
  else if (A.D <= 32)
    hipLaunchKernelGGL((glp_f64_kernel<32, 32, 4, E64>), grid, dim3(256), 0, s, A);
  else
    hipLaunchKernelGGL((glp_f64_kernel<64, 32, 2, E64>), grid, dim3(128), 0, s, A);
}

extern "C" {

int64_t hbx_kde_logpdf_groups_workspace_bytes(int64_t B, int64_t C, int32_t D) {
  if (D < 1 || D > HBX_MAX_D || !glp_counts_ok(B, C)) return -1;
  return GLP_HEAD + glp_cnt_bytes(B) + B * C * 2 * (int64_t)sizeof(int32_t);
}

int hbx_kde_logpdf_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                          const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad, const double* cand,
                          int64_t C, double rtol, int32_t flags, double* ln_l, double* ln_g, int32_t* status,
                          void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_logpdf_groups";
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || C < 0) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld", who, (long long)B, (long long)C);
  if (!glp_counts_ok(B, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * C = %lld * %lld exceeds int32", who, (long long)B, (long long)C);
  if (!(rtol > 0.0)) return hbx_fail(HBX_ERR_ARG, "%s: rtol=%g must be positive", who, rtol);
  if (flags & ~HBX_LOGPDF_FP64_ONLY) return hbx_fail(HBX_ERR_ARG, "%s: flags=%d", who, flags);
  if (!ln_l && !ln_g) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (ln_l and ln_g)", who);
  if (B == 0 || C == 0) return HBX_OK;
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !bw_good || !bw_bad || !nlev_good || !nlev_bad ||
      !cand || !status || !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const uintptr_t a8 = (uintptr_t)X | (uintptr_t)seg_off | (uintptr_t)order | (uintptr_t)n_good | (uintptr_t)n_bad |
                       (uintptr_t)bw_good | (uintptr_t)bw_bad | (uintptr_t)cand | (uintptr_t)ln_l | (uintptr_t)ln_g;
  const uintptr_t a4 = (uintptr_t)vartype | (uintptr_t)nlev_good | (uintptr_t)nlev_bad | (uintptr_t)status;
  if ((a8 & 7) || (a4 & 3) || ((uintptr_t)workspace & 15))
    return hbx_fail(HBX_ERR_ARG, "%s: pointers must be aligned (f64 / i64: 8 bytes, i32: 4, workspace: 16)", who);
  const int64_t need = hbx_kde_logpdf_groups_workspace_bytes(B, C, D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  GlpArgs A;
  A.X = X;
  A.seg_off = seg_off;
  A.order = order;
  A.n_good = n_good;
  A.n_bad = n_bad;
  A.vartype = vartype;
  A.bw_good = bw_good;
  A.bw_bad = bw_bad;
  A.nlev_good = nlev_good;
  A.nlev_bad = nlev_bad;
  A.cand = cand;
  A.B = B;
  A.C = C;
  A.D = D;
  A.tiles = (int32_t)((C + 63) / 64);
  A.dcp = D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;  // the slot bucket, from D alone (vartype is device memory)
  A.dup = D <= 8 ? 8 : D <= 16 ? 16 : 32;
  A.kd0 = ln_l ? 0 : 1;
  A.fp64_only = (flags & HBX_LOGPDF_FP64_ONLY) ? 1 : 0;
  A.rtol = rtol;
  A.out[0] = ln_l;
  A.out[1] = ln_g;
  A.status = status;
  A.stat = (unsigned long long*)workspace;
  A.cnt = (int32_t*)((char*)workspace + GLP_HEAD);
  A.list = (int32_t*)((char*)workspace + GLP_HEAD + glp_cnt_bytes(B));
  HBX_HIP(hipMemsetAsync(workspace, 0, (size_t)(GLP_HEAD + glp_cnt_bytes(B)), s));
  hipLaunchKernelGGL(glp_status_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, A);
  HBX_LAUNCH_CHECK();
  const dim3 grid((unsigned)(B * A.tiles), (ln_l && ln_g) ? 2u : 1u);  // B * tiles <= B * C <= INT32_MAX
  if (!A.fp64_only) {
    if (D <= 8)
      hipLaunchKernelGGL((glp_dd_kernel<8, 8, 4, 16>), grid, dim3(256), 0, s, A);
    else if (D <= 16)
      hipLaunchKernelGGL((glp_dd_kernel<16, 16, 4, 24>), grid, dim3(256), 0, s, A);
    else if (D <= 32)
      hipLaunchKernelGGL((glp_dd_kernel<32, 32, 4, 40>), grid, dim3(256), 0, s, A);
    else  // D <= 96 with <= 64 continuous and <= 32 categorical dims; anything larger is EXACT
      hipLaunchKernelGGL((glp_dd_kernel<64, 32, 2, 104>), grid, dim3(128), 0, s, A);
    HBX_LAUNCH_CHECK();
  }
  if (rtol < 1e-5)
    glp_launch_f64<true>(A, grid, s);
  else
    glp_launch_f64<false>(A, grid, s);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(glp_exact_kernel, grid, dim3(EXACT_THREADS), 0, s, A);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int hbx_kde_logpdf_groups_stats(const void* workspace, int64_t* out4) {
  if (!workspace || !out4) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf_groups_stats: null pointer");
  unsigned long long st[4];
  HBX_HIP(hipDeviceSynchronize());
  HBX_HIP(hipMemcpy(st, workspace, sizeof(st), hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k) out4[k] = (int64_t)st[k];
  return HBX_OK;
}

}  // extern "C"
