// hbx_groups_impl.h -- what the grouped kernels share: the grouped counterpart of hbx_acq_impl.h / hbx_exact_impl.h.
// hbx_groups.hip (the two screens, the select, the top-k) and hbx_groups_logpdf.hip (the fp32 pass, the exact pass)
// include it; hbx_groups_config.hip includes it for the count rule alone.  Every statement that carries part of a
// written error bound -- a, b, dd, the fma chain, the |b| maxima taken while staging -- stands here once:
//   GrpModel, grp_model        the model as hbx_kde_fit leaves it on the device, and the slot bucket from D
//   grp_classify               what kind of group b is, per KDE; the callers map it to their own status bits
//   grp_slots                  the dims sorted into slots by one wave
//   GrpLayout, grp_layout      the layout of a staged row and the piece counts of the pair loop
//   GrpConsts, GrpScreenConsts the per-group constants of one or both KDEs in LDS, grp_consts_fill / grp_screen_sums
//   grp_stage<SL>              one wave stages jmax rows of one KDE: gather, centre, scale, fp32, |b| maxima
//   grp_load_cand              a lane's candidate against one KDE, in registers
//   grp_pair_t                 the pair exponent t (and the parity of a signed term) for one staged row
//   grp_pairs, GRP_PAIRS_DISPATCH   the screens' running log-sum-exp over a chunk; the dispatch over the piece counts
//   grp_estimate, grp_emit, grp_uncertified   sums -> KdeEst with its bound -> GScreen
//   GrpView, grp_view          the per-group parameter view of the exact functions
//   grp_compact, grp_exact_both     a 256-candidate chunk's shortlist; both exact pdfs of one entry
//   grp_counts_ok, grp_check_dim, grp_model_null, grp_model_misaligned    the host checks
//
// The pair exponent, in log2 units (fp32, direct differences -- no expansion, so no cancellation):
//     t_ij = t0 + sum_c -(a_ic - b_jc)^2 + sum_u m_iju delta_u,      a = fl(s_c (x_c - mu_c)), b = fl(s_c (X_jc - mu_c))
//   s_c = sqrt(log2 e / 2) / h_c, mu_c = mean of the group's first <= 64 good rows (any centre is exact algebra; this
//   one keeps |a|, |b| small), m = [x_u == X_ju], lb = sum_u log2(h_u / (c_u - 1)), delta_u = log2|1 - h_u| - log2(h_u /
//   (c_u - 1)) (-1e30 where 1 - h_u == 0: the term is exactly 0).  The screens start the chain at t0 = fl(lb); the
//   ln-pdf at 0 and adds lb in fp64 at the end.  A categorical h > 1 makes the match factor negative: the term's sign
//   is the parity of its matches in such dims.
//
// The screens' error bound (u = 2^-24), per candidate i and KDE, with A_c = |a_ic|, B_c = max_j |b_jc| (taken while
// staging, grp_stage), R_c = A_c + B_c -- evaluated by grp_estimate:
//     - a and b are fp64 products rounded once: |a - a*| <= u |a*|, |b - b*| <= u |b*| (the fp64 roundings of s, of the
//       subtraction and of the product are 2^-29 of that and sit in the 1.02 below); dd = fl(a - b) adds u |a - b|.
//       So |dd - d*| <= 2.02 u R_c, |dd + d*| <= 2.01 R_c and |dd^2 - d*^2| <= 4.1 u R_c^2.
//     - t is a chain of dc + du fma steps from fl(lb), one rounding each of at most u |partial|, and every partial
//       is bounded by T = |lb| + sum_c R_c^2 + sum_u |delta_u| (finite deltas); fl(lb) and fl(delta_u) add u (|lb| +
//       sum |delta_u|); m is exact (integer codes below 2^24).
//     => |t - t*| <= E_t = 1.02 u (dc + du + 8) T.  A term's weight is off by a factor within 2^+-E_t, and
//       2^E - 1 <= 1.05 E for E <= 0.5; candidates with E_t > 0.5 (or any non-finite coordinate or sum) are not
//       certified and are shortlisted unconditionally.
//     - the sums (grp_pairs): rescaling is exact (integer exponents; a flush below 2^-126 is beyond the slack).  A term
//       e = exp2(fl(t - m)): the argument's rounding u |t - m| changes e by at most 0.7 u |t - m| 2^-|t - m| <= 0.372 u,
//       v_exp_f32 by 2 u e; with the largest term in (1/2, 1] the sum is >= 1/2, so n terms add at most (2 + 0.75 n) u
//       relative, their n additions n u, a merge of NW waves' sums NW more.
//     => err = 1.05 E_t + (2 n + 40) u (32 for the merge and the flushes, 8 for log2 of the sum), relative, per sum,
//       against S+ + S-: exactly what est_interval() expects; its own slack covers the final rounding to float.
// The ln-pdf's bound shares the coordinates' part (a, b, dd, B_c) and is derived in hbx_groups_logpdf.hip.
#pragma once
#include <math.h>

#include "hbx_acq_impl.h"
#include "hbx_exact_impl.h"

// ---- the model --------------------------------------------------------------------------------------------
// Inputs are hbx_kde_fit's, as they lie on the device: group b's rows are X[seg_off[b] + order[seg_off[b] + j]], good
// KDE j < n_good[b], bad KDE j in [n - n_bad[b], n); its bandwidths and level counts are bw_*[b][D], nlev_*[b][D].
struct GrpModel {
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
  int64_t B;
  int32_t D;
  int32_t dcp, dup;  // the slot bucket
};

// The slot bucket comes from D alone (vartype is device memory): D <= 8, 16, 32 -> every dim may be of either kind
// (DCP = DUP = the bucket); D <= 96 -> up to 64 continuous and 32 categorical; anything larger is exact-only.
static inline GrpModel grp_model(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                 const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                 const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                 const int32_t* nlev_bad) {
  GrpModel M;
  M.X = X;
  M.seg_off = seg_off;
  M.order = order;
  M.n_good = n_good;
  M.n_bad = n_bad;
  M.vartype = vartype;
  M.bw_good = bw_good;
  M.bw_bad = bw_bad;
  M.nlev_good = nlev_good;
  M.nlev_bad = nlev_bad;
  M.B = B;
  M.D = D;
  M.dcp = D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
  M.dup = D <= 8 ? 8 : D <= 16 ? 16 : 32;
  return M;
}

// the launch of the bucket's instance of a kernel template <DCP, DUP, NW, DT>: LAUNCH(DCP, DUP, NW, DT)
#define GRP_BUCKET_LAUNCH(D, LAUNCH) \
  do {                               \
    if ((D) <= 8)                    \
      LAUNCH(8, 8, 4, 16);           \
    else if ((D) <= 16)              \
      LAUNCH(16, 16, 4, 24);         \
    else if ((D) <= 32)              \
      LAUNCH(32, 32, 4, 40);         \
    else                             \
      LAUNCH(64, 32, 2, 104);        \
  } while (0)

// ---- classification ---------------------------------------------------------------------------------------
#define GRP_NO_MODEL 1
#define GRP_UNSUPPORTED 2
#define GRP_EXACT(kd) (4 << (kd))  // KDE kd (0 good, 1 bad) cannot be screened: only the exact fp64 pdf says what it is
#define GRP_NEG(kd) (16 << (kd))   // KDE kd has a negative categorical match factor (h > 1)
#define GRP_EXACT_ANY (GRP_EXACT(0) | GRP_EXACT(1))

// What kind of group b is: hbx_kde_fit's skip rule, hbx_kde_prepare's per-dim rules, the bucket.  Called by one whole
// wave (lane = dim, 64 dims at a time); every lane returns the same bits and counts.  GRP_NO_MODEL comes alone.
__device__ __forceinline__ int grp_classify(const GrpModel& M, int64_t b, int* dc_out, int* du_out) {
  const int64_t n = M.seg_off[b + 1] - M.seg_off[b], ng = M.n_good[b], nb = M.n_bad[b];
  *dc_out = *du_out = 0;
  if (ng <= 0 || ng > n || nb <= 0 || nb > n) return GRP_NO_MODEL;  // (uniform)
  const int lane = threadIdx.x & 63;
  int st = 0, dc = 0, du = 0;
  for (int d0 = 0; d0 < M.D; d0 += 64) {
    const int d = d0 + lane;
    const bool live = d < M.D;
    const bool cont = live && M.vartype[d] == 0;
    dc += __popcll(__ballot(cont));
    du += __popcll(__ballot(live && !cont));
    if (!live) continue;
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {
      const double h = (kd ? M.bw_bad : M.bw_good)[b * M.D + d];
      if (cont) {
        if (!(h > 0.0 && h < INFINITY)) st |= GRP_EXACT(kd);  // pdf NaN (or 0) everywhere: the exact path says which
      } else {
        const int c = (kd ? M.nlev_bad : M.nlev_good)[b * M.D + d];
        if (c == 1 && (h == 0.0 || (h > 0.0 && h < INFINITY)))
          // one observed level: match -> 1, mismatch -> 0 / 0; under a finite h > 0 (a fitted 0 clipped to
          // hbx_rules.min_bandwidth): match -> 1 - h, mismatch -> h / 0 = +inf -- hbx_kde_prepare's rule
          st |= GRP_EXACT(kd);
        else if (c < 2 || !(h > 0.0) || h != h)
          st |= GRP_UNSUPPORTED;  // (c == -1: codes not integers in [0, 1024))
        else if (!(h < INFINITY))
          st |= GRP_EXACT(kd);
        else if (1.0 - h < 0.0)
          st |= GRP_NEG(kd);
      }
    }
  }
  st = (int)wave_reduce_dpp((uint32_t)st, OpOr());
  if (dc > M.dcp || du > M.dup) st |= GRP_EXACT_ANY;  // the dims exceed the bucket
  *dc_out = dc;
  *du_out = du;
  return st;
}

// The dims of a usable group sorted into slots in dim order by one wave: continuous dims to cdim[0 .. dc), categorical
// dims to udim[0 .. du); every lane returns the counts (the caller has checked dc <= DCP, du <= DUP: grp_classify).
__device__ __forceinline__ void grp_slots(const GrpModel& M, int lane, int32_t* cdim, int32_t* udim, int* dc, int* du) {
  int kc = 0, ku = 0;
  for (int d0 = 0; d0 < M.D; d0 += 64) {
    const int d = d0 + lane;
    const bool cont = d < M.D && M.vartype[d] == 0, cat = d < M.D && !cont;
    const uint64_t mc = __ballot(cont), mu = __ballot(cat), below = (1ull << lane) - 1ull;
    if (cont) cdim[kc + __popcll(mc & below)] = d;
    if (cat) udim[ku + __popcll(mu & below)] = d;
    kc += __popcll(mc);
    ku += __popcll(mu);
  }
  *dc = kc;
  *du = ku;
}

// ---- the row layout ---------------------------------------------------------------------------------------
// A staged row (stride rs floats): continuous slots from 0, categorical slots from dc4 = 4 dcq.  Compile-time piece
// counts serve dc <= 32 in qcs = 2 / 4 / 6 / 8 pieces with du <= 8 in 0 / 2 pieces (config #5's 24c + 8u: 6 + 2), where
// the instance has the slots for them (`fast`); everything else takes the exact piece counts dcq, duq.
struct GrpLayout {
  int qcs, dcq, duq, dc4, du4;
  int rs;   // <= DT + 4
  int rpp;  // rows per staging pass
  bool fast;
};
template <int DCP, int DUP>
__device__ __forceinline__ GrpLayout grp_layout(int D, int dc, int du) {
  GrpLayout L;
  L.qcs = dc <= 8 ? 2 : dc <= 16 ? 4 : dc <= 24 ? 6 : 8;
  L.fast = dc <= 32 && du <= 8 && 4 * L.qcs <= DCP && DUP >= 8;
  L.dcq = L.fast ? L.qcs : (dc + 3) >> 2;
  L.duq = L.fast ? (du ? 2 : 0) : (du + 3) >> 2;
  L.dc4 = 4 * L.dcq;
  L.du4 = 4 * L.duq;
  L.rs = L.dc4 + L.du4 + 4;
  L.rpp = D <= 64 ? 64 / D : 1;
  return L;
}

// ---- per-group constants ----------------------------------------------------------------------------------
// The constants of NK KDEs of one group, placed in LDS by the kernel: NK = 2 holds the good KDE at index 0 and the bad
// one at 1; NK = 1 holds KDE kd0.  (The |b| maxima stay outside: their shape differs between the kernels.)
// The struct holds pointers to LDS arrays that the kernel declares one by one (GRP_CONSTS_LDS / GRP_SCREEN_CONSTS_LDS),
// not the arrays themselves: with the arrays as members of one LDS object -- the same bytes at the same size, nothing
// else changed -- the compiler combines and schedules their reads differently, and groups_screen_kernel came out at 173
// instead of 165 VGPRs in the 8-slot instance (two waves per SIMD instead of three) and at 256 VGPRs + 4 AGPRs instead
// of 255 in the 32-slot one (one wave instead of two).  Pointers to separate arrays fold away when the functions inline.
template <int DCP, int DUP, int NK>
struct GrpConsts {
  static constexpr int dcp = DCP, dup = DUP, nk = NK;
  static constexpr bool screen = false;
  int32_t *cdim, *udim;  // slot -> dim
  int32_t* doff;         // dim -> float offset of its slot in a staged row
  double *mu, (*scale)[DCP];
  double *dmu, (*dsc)[DCP + DUP];  // dim -> centre (categorical: 0) and scale (1)
  float (*delta)[DUP];
};
// GRP_CONSTS_LDS(K, ...) declares the LDS arrays in the kernel and K with its pointers set to them
#define GRP_CONSTS_ARRAYS_(K, DCP, DUP, NK)                                                            \
  __shared__ int32_t K##_cdim[DCP], K##_udim[DUP], K##_doff[DCP + DUP];                                \
  __shared__ double K##_mu[DCP], K##_scale[NK][DCP], K##_dmu[DCP + DUP], K##_dsc[NK][DCP + DUP];       \
  __shared__ float K##_delta[NK][DUP];                                                                 \
  K.cdim = K##_cdim, K.udim = K##_udim, K.doff = K##_doff, K.mu = K##_mu, K.scale = K##_scale;         \
  K.dmu = K##_dmu, K.dsc = K##_dsc, K.delta = K##_delta
#define GRP_CONSTS_LDS(K, DCP, DUP, NK) \
  GrpConsts<DCP, DUP, NK> K;            \
  GRP_CONSTS_ARRAYS_(K, DCP, DUP, NK)
// ... and what the screens need beyond that: the pieces of the norms and of lb for the deterministic sums
// (grp_screen_sums), the sign flags, and the sums themselves.  The ln-pdf's fp32 pass keeps its own sums (in ln units
// and fp64, hbx_groups_logpdf.hip), so it does not carry these arrays in LDS.
template <int DCP, int DUP>
struct GrpScreenConsts : GrpConsts<DCP, DUP, 2> {
  static constexpr bool screen = true;
  double (*lnh)[DCP], (*lb)[DUP];
  float (*negf)[DUP];
  double* norm;
  float *lbs, *tfix;
};
#define GRP_SCREEN_CONSTS_LDS(K, DCP, DUP)                                  \
  GrpScreenConsts<DCP, DUP> K;                                              \
  GRP_CONSTS_ARRAYS_(K, DCP, DUP, 2);                                       \
  __shared__ double K##_lnh[2][DCP], K##_lb[2][DUP], K##_norm[2];           \
  __shared__ float K##_negf[2][DUP], K##_lbs[2], K##_tfix[2];               \
  K.lnh = K##_lnh, K.lb = K##_lb, K.negf = K##_negf, K.norm = K##_norm, K.lbs = K##_lbs, K.tfix = K##_tfix

// The per-slot constants of KDEs kd0 .. kd0 + NK - 1 of group b, by the whole block of NT threads (cdim, udim filled;
// a barrier before and after is the caller's).  A GrpScreenConsts gets its lnh, lb and negf filled too.
template <int NT, class KT>
__device__ __forceinline__ void grp_consts_fill(KT& K, const GrpModel& M, int64_t b, int kd0, int dc, int du, int dc4,
                                                int tid) {
  constexpr int DCP = KT::dcp, DUP = KT::dup, NK = KT::nk;
  constexpr bool SCREEN = KT::screen;
  const int D = M.D;
  const int64_t s0 = M.seg_off[b], ng = M.n_good[b];
  const double* Xs = M.X + s0 * D;
  const int64_t* ord = M.order + s0;
  for (int k = tid; k < DCP; k += NT) {
    if (k < dc) {
      const int d = K.cdim[k];
      const int nm = (int)(ng < 64 ? ng : 64);
      double sum = 0.0;
#pragma unroll 16
      for (int j = 0; j < nm; ++j) sum += Xs[ord[j] * D + d];
      double mu = sum / (double)nm;
      if (!(mu - mu == 0.0)) mu = 0.0;
      K.mu[k] = mu;
      K.dmu[d] = mu;
      K.doff[d] = k;
#pragma unroll
      for (int q = 0; q < NK; ++q) {
        const double h = ((kd0 + q) ? M.bw_bad : M.bw_good)[b * D + d];
        K.scale[q][k] = sqrt(M_LOG2E / 2.0) / h;
        K.dsc[q][d] = K.scale[q][k];
        if constexpr (SCREEN) K.lnh[q][k] = log(h);
      }
    } else {
      K.mu[k] = 0.0;
#pragma unroll
      for (int q = 0; q < NK; ++q) K.scale[q][k] = 0.0;
    }
  }
  for (int u = tid; u < DUP; u += NT) {
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      float dl = 0.f, ngf = 0.f;
      double lb = 0.0;
      if (u < du) {
        const int d = K.udim[u];
        K.doff[d] = dc4 + u;
        K.dsc[q][d] = 1.0;
        K.dmu[d] = 0.0;
        const double h = ((kd0 + q) ? M.bw_bad : M.bw_good)[b * D + d];
        const int c = ((kd0 + q) ? M.nlev_bad : M.nlev_good)[b * D + d];
        const double a = 1.0 - h;
        lb = log2(h / (double)(c - 1));
        dl = (a == 0.0) ? -1e30f : (float)(log2(fabs(a)) - lb);
        ngf = a < 0.0 ? 1.f : 0.f;
      }
      K.delta[q][u] = dl;
      if constexpr (SCREEN) {
        K.negf[q][u] = ngf;
        K.lb[q][u] = lb;
      }
    }
  }
}

// the screens' sums in slot order (deterministic), by threads 0 and 1: the norm -ln n - sum_c ln(h_c sqrt(2 pi)), lb,
// and |lb| + sum |delta| for the bound
template <int DCP, int DUP>
__device__ __forceinline__ void grp_screen_sums(GrpScreenConsts<DCP, DUP>& K, int dc, int du, int64_t ng, int64_t nb,
                                                int tid) {
  if (tid < 2) {
    const int kd = tid;
    double sl = 0.0, lb = 0.0;
    float sad = 0.f;
    for (int k = 0; k < dc; ++k) sl += K.lnh[kd][k];
    for (int u = 0; u < du; ++u) {
      lb += K.lb[kd][u];
      if (K.delta[kd][u] > -1e29f) sad += fabsf(K.delta[kd][u]);
    }
    K.norm[kd] = -log((double)(kd ? nb : ng)) - sl - 0.5 * (double)dc * log(2.0 * M_PI);
    K.lbs[kd] = (float)lb;
    K.tfix[kd] = (fabsf((float)lb) + sad) * 1.0001f;  // |lb| + sum |delta|
  }
}

// ---- staging ----------------------------------------------------------------------------------------------
// One wave stages rows[j0 .. j0 + jmax) of one KDE (jmax <= 64) into wrows as fp32, centred and scaled (dsc: the
// KDE's dim -> scale), and raises bmax[slot] to the rows' |b| maxima.  lane = (row in pass, dim): a row's D doubles are
// read by consecutive lanes (coalesced), SL passes of loads in flight; dims past 64 take further rounds (db).  The
// chunk's row positions come in one coalesced load and reach the lanes by a lane exchange (no dependent global load
// per pass).
template <int SL>
__device__ __forceinline__ void grp_stage(const double* __restrict__ Xs, int D, const int64_t* __restrict__ rows,
                                          int64_t j0, int jmax, float* __restrict__ wrows, int rs, int rpp, int dc,
                                          const int32_t* doff, const double* dsc, const double* dmu, uint32_t* bmax,
                                          int lane) {
  const int myrow = (int)rows[j0 + (lane < jmax ? lane : 0)];  // (positions local to the segment: < 2^31)
  for (int db = 0; db < D; db += 64) {
    const int lr = D <= 64 ? lane / D : 0;
    const int ld = db + (D <= 64 ? lane - lr * D : lane);
    const bool act = lr < rpp && ld < D;
    const int off = act ? doff[ld] : 0;
    const double sc = act ? dsc[ld] : 0.0, mu = act ? dmu[ld] : 0.0;
    uint32_t bm = 0u;  // |b| maximum of this lane's dim (non-negative floats order as their bits; NaN above all)
    for (int p0 = 0; p0 < jmax; p0 += SL * rpp) {
      double t[SL];
#pragma unroll
      for (int q = 0; q < SL; ++q) {
        const int r = p0 + q * rpp + lr;
        const int ri = __shfl(myrow, r < jmax ? r : 0);  // (every lane takes part in the exchange)
        t[q] = (act && r < jmax) ? Xs[(int64_t)ri * D + ld] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < SL; ++q) {
        const int r = p0 + q * rpp + lr;
        if (act && r < jmax) {
          const float v = (float)(sc * (t[q] - mu));
          wrows[r * rs + off] = v;
          bm = max(bm, __float_as_uint(fabsf(v)));
        }
      }
    }
    if (act && off < dc) atomicMax(&bmax[off], bm);
  }
}

// ---- a lane's candidate -----------------------------------------------------------------------------------
__device__ __forceinline__ float grp_uniform(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// This lane's candidate x against one KDE (scale, delta: that KDE's rows of the constants): its scaled coordinates,
// its codes and the KDE's deltas in registers; a non-finite coordinate clears `certified`.
template <int DCP, int DUP>
__device__ __forceinline__ void grp_load_cand(const double* __restrict__ x, int dc, int du, const int32_t* cdim,
                                              const int32_t* udim, const double* scale, const double* mu,
                                              const float* delta, float (&xc)[DCP], float (&xu)[DUP], float (&dl)[DUP],
                                              bool& certified) {
#pragma unroll
  for (int k = 0; k < DCP; ++k) {
    xc[k] = 0.f;
    if (k < dc) {
      const double xv = x[cdim[k]];
      certified = certified && (xv - xv == 0.0);
      xc[k] = (float)(scale[k] * (xv - mu[k]));
    }
  }
#pragma unroll
  for (int u = 0; u < DUP; ++u) {
    xu[u] = 0.f;
    if (u < du) {
      const double xv = x[udim[u]];
      certified = certified && (xv - xv == 0.0);
      xu[u] = cand_code(xv);
    }
    dl[u] = grp_uniform(delta[u]);
  }
}

// ---- the pair exponent ------------------------------------------------------------------------------------
// t of this lane's candidate against the staged row rj, from t0 (header).  QC >= 0: QC continuous and QU categorical
// 4-slot pieces, compile-time counts (the padding slots are zeros on both sides: a zero difference, a match with delta
// 0); every LDS read of the row is issued before its first use -- with uniform branches between them the compiler waits
// for each read on its own, one LDS latency per piece instead of one per pair.  QC < 0: dcq / duq pieces with a uniform
// branch each.  SG: *par counts the matches in dims with a negative factor (nf: their flags); nf is not read otherwise.
template <int DCP, int DUP, int QC, int QU, bool SG>
__device__ __forceinline__ float grp_pair_t(const float4* __restrict__ rj, int dcq, int duq, const float (&xc)[DCP],
                                            const float (&xu)[DUP], const float (&dl)[DUP], const float* nf, float t0,
                                            float* par) {
  float t = t0, p = 0.f;
  auto cont4 = [&](int q, const float4 v) {
    const float d0 = xc[4 * q] - v.x, d1 = xc[4 * q + 1] - v.y, d2 = xc[4 * q + 2] - v.z, d3 = xc[4 * q + 3] - v.w;
    t = fmaf(-d0, d0, t);
    t = fmaf(-d1, d1, t);
    t = fmaf(-d2, d2, t);
    t = fmaf(-d3, d3, t);
  };
  auto cat4 = [&](int q, const float4 v) {
    const float m0 = cat_match(xu[4 * q], v.x), m1 = cat_match(xu[4 * q + 1], v.y);
    const float m2 = cat_match(xu[4 * q + 2], v.z), m3 = cat_match(xu[4 * q + 3], v.w);
    t = fmaf(m0, dl[4 * q], t);
    t = fmaf(m1, dl[4 * q + 1], t);
    t = fmaf(m2, dl[4 * q + 2], t);
    t = fmaf(m3, dl[4 * q + 3], t);
    if constexpr (SG) {
      p = fmaf(m0, nf[4 * q], p);
      p = fmaf(m1, nf[4 * q + 1], p);
      p = fmaf(m2, nf[4 * q + 2], p);
      p = fmaf(m3, nf[4 * q + 3], p);
    }
  };
  if constexpr (QC >= 0) {
    static_assert(4 * QC <= DCP && 4 * QU <= DUP, "pieces within the slots");
    float4 vc[QC > 0 ? QC : 1], vu[QU > 0 ? QU : 1];
#pragma unroll
    for (int q = 0; q < QC; ++q) vc[q] = rj[q];
#pragma unroll
    for (int q = 0; q < QU; ++q) vu[q] = rj[QC + q];
#pragma unroll
    for (int q = 0; q < QC; ++q) cont4(q, vc[q]);
#pragma unroll
    for (int q = 0; q < QU; ++q) cat4(q, vu[q]);
  } else {
#pragma unroll
    for (int q = 0; q < DCP / 4; ++q)
      if (q < dcq) cont4(q, rj[q]);  // uniform
#pragma unroll
    for (int q = 0; q < DUP / 4; ++q)
      if (q < duq) cat4(q, rj[dcq + q]);  // uniform
  }
  if constexpr (SG) *par = p;
  return t;
}

// One staged chunk's pairs for this lane's candidate, the screens' sum: rows[0 .. jmax) of stride rs.  Running
// log-sum-exp with an INTEGER running maximum m = max ceil(t): the sums S+-, in units of 2^m, are rescaled by ldexp
// (exact), each term adds exp2(t - m); positive and negative terms are summed apart.
template <int DCP, int DUP, int QC, int QU, bool SG>
__device__ __forceinline__ void grp_pairs(const float* __restrict__ rows, int rs, int jmax, int dcq, int duq,
                                          const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                          const float (&nf)[DUP], float lbs, float& m, float& sp, float& sn) {
  for (int j = 0; j < jmax; ++j) {
    float par = 0.f;
    const float t = grp_pair_t<DCP, DUP, QC, QU, SG>((const float4*)(rows + j * rs), dcq, duq, xc, xu, dl, nf, lbs, &par);
    const float tc = ceilf(t);
    if (tc > m) {  // a new running maximum (integer): exact rescale
      const int sh = (int)fmaxf(m - tc, -250.f);
      sp = ldexpf(sp, sh);
      if (SG) sn = ldexpf(sn, sh);
      m = tc;
    }
    const float e = __builtin_amdgcn_exp2f(t - m);
    if (SG) {
      const bool odd = ((int)par) & 1;
      sp += odd ? 0.f : e;
      sn += odd ? e : 0.f;
    } else {
      sp += e;
    }
  }
}

// The dispatch over the piece counts.  GRP_PAIRS_DISPATCH: F(QC, QU, SG) with the layout's compile-time counts where
// it has them -- qcs continuous pieces, no categorical piece (cat == 0), two (cat == 1), two with signed terms
// (cat == 2) -- and F(-1, -1, SG) otherwise.  GRP_PAIRS_DISPATCH_UNSIGNED: the same for sums without signed terms
// (cat is 0 or 1), F(QC, QU).  DCP bounds the instances: one that the bucket cannot reach is not compiled.
#define GRP_PAIRS_BY_QC_(DCP, L, CAT, REST, cat, F)  \
  do {                                               \
    if ((L).fast && (L).qcs == 2) {                  \
      CAT(2, cat, F);                                \
    } else if ((L).fast && (L).qcs == 4) {           \
      if constexpr (DCP >= 16) CAT(4, cat, F);       \
    } else if ((L).fast && (L).qcs == 6) {           \
      if constexpr (DCP >= 24) CAT(6, cat, F);       \
    } else if ((L).fast) {                           \
      if constexpr (DCP >= 32) CAT(8, cat, F);       \
    } else {                                         \
      REST(cat, F);                                  \
    }                                                \
  } while (0)
#define GRP_PAIRS_CAT_(QC, cat, F) \
  do {                             \
    if ((cat) == 0)                \
      F(QC, 0, false);             \
    else if ((cat) == 1)           \
      F(QC, 2, false);             \
    else                           \
      F(QC, 2, true);              \
  } while (0)
#define GRP_PAIRS_REST_(cat, F) \
  do {                          \
    if ((cat) == 2)             \
      F(-1, -1, true);          \
    else                        \
      F(-1, -1, false);         \
  } while (0)
#define GRP_PAIRS_CAT_UNSIGNED_(QC, cat, F) \
  do {                                      \
    if ((cat) == 0)                         \
      F(QC, 0);                             \
    else                                    \
      F(QC, 2);                             \
  } while (0)
#define GRP_PAIRS_REST_UNSIGNED_(cat, F) F(-1, -1)
#define GRP_PAIRS_DISPATCH(DCP, L, cat, F) GRP_PAIRS_BY_QC_(DCP, L, GRP_PAIRS_CAT_, GRP_PAIRS_REST_, cat, F)
#define GRP_PAIRS_DISPATCH_UNSIGNED(DCP, L, cat, F) \
  GRP_PAIRS_BY_QC_(DCP, L, GRP_PAIRS_CAT_UNSIGNED_, GRP_PAIRS_REST_UNSIGNED_, cat, F)

// ---- the screens' estimate and record ------------------------------------------------------------------------
struct GScreen {
  union {
    struct {
      float slo, shi;  // ln score interval ...
    };
    double score;  // ... and after the re-score (GS_DONE) the exact fp64 score in the same 8 bytes
  };
  float rel;  // bound of |score here - score in numpy's arithmetic| / score (exact_rel of both pdfs)
  uint32_t fl;
};
static_assert(sizeof(GScreen) == 16, "one 16-byte slot per candidate");
#define GS_FORCE 1u  // bound not certified: re-scored unconditionally
#define GS_ONE 2u    // score certainly exactly 1
#define GS_OF 4u     // a pdf bound past fp64's exp range: the group is re-scored whole
#define GS_DONE 8u   // re-scored: the first 8 bytes are the exact score

// exact_rel (hbx_acq_impl.h) without a KdeParams block: est == nullptr -> no estimate of the condition
__device__ __forceinline__ double grp_exact_rel(int D, bool has_neg, const KdeEst* est) {
  const double base = (8.0 * (double)D + 160.0) * 0x1p-52;
  if (!has_neg) return base;
  if (!est) return INFINITY;
  const KdeEst e = *est;
  const float m = fmaxf(e.lpos, e.lneg);
  if (!(m > -INFINITY)) return base;
  const float a = __expf(e.lpos - m), b = __expf(e.lneg - m);
  const float den = fabsf(a - b) - (e.err + 1e-6f) * (a + b);
  if (!(den > 0.f)) return INFINITY;
  return base * (double)((a + b) / den) * 1.01;
}

// The candidate's sums over KDE kd's nk rows (Sp, Sn in units of 2^M) -> KdeEst with the header's bound; bmax: the
// KDE's |b| maxima, complete.  `bad`: a NaN among the running maxima.
template <int DCP, int DUP>
__device__ __forceinline__ KdeEst grp_estimate(const GrpScreenConsts<DCP, DUP>& K, int kd, int dc, int du, int64_t nk,
                                               const uint32_t* bmax, const float (&xc)[DCP], float M, float Sp,
                                               float Sn, bool bad, bool& certified) {
  float T = K.tfix[kd];
#pragma unroll
  for (int k = 0; k < DCP; ++k)
    if (k < dc) {
      const float r = fabsf(xc[k]) + __uint_as_float(bmax[k]);
      T = fmaf(r, r, T);
    }
  const float u24 = 0x1p-24f;
  const float Et = 1.02f * u24 * (float)(dc + du + 8) * T;
  KdeEst e;
  e.pad = 0.f;
  e.err = 1.05f * Et + (2.f * (float)nk + 40.f) * u24;
  if (!(Et < 0.5f) || bad || !(Sp - Sp == 0.f) || !(Sn - Sn == 0.f) || !(M - M == 0.f)) certified = false;
  const double nrm = K.norm[kd];
  e.lpos = Sp > 0.f ? (float)(((double)__log2f(Sp) + (double)M) * M_LN2 + nrm) : -INFINITY;
  e.lneg = Sn > 0.f ? (float)(((double)__log2f(Sn) + (double)M) * M_LN2 + nrm) : -INFINITY;
  return e;
}

// the slot of a candidate without a certified bound: re-scored unconditionally (st: grp_classify's bits)
__device__ __forceinline__ GScreen grp_uncertified(int D, int st) {
  GScreen g;
  g.slo = g.shi = NAN;
  g.rel = (float)((grp_exact_rel(D, st & GRP_NEG(0), nullptr) + grp_exact_rel(D, st & GRP_NEG(1), nullptr) + 0x1p-51) *
                  1.000001);
  g.fl = GS_FORCE;
  return g;
}

// both estimates -> score_interval() (hbx_acq_impl.h) unchanged, under the call's score floor -> the candidate's slot
__device__ __forceinline__ GScreen grp_emit(int D, int st, bool certified, const KdeEst& est_l, const KdeEst& est_g,
                                            const ScoreFloor F) {
  if (!certified) return grp_uncertified(D, st);
  GScreen g;
  const ScoreIv v = score_interval(est_l, est_g, F);
  g.slo = v.slo;
  g.shi = v.shi;
  g.rel = (float)((grp_exact_rel(D, st & GRP_NEG(0), &est_l) + grp_exact_rel(D, st & GRP_NEG(1), &est_g) + 0x1p-51) *
                  1.000001);
  g.fl = (v.one ? GS_ONE : 0u) | (v.of ? GS_OF : 0u) | ((v.lnan || v.slo != v.slo || v.shi != v.shi) ? GS_FORCE : 0u);
  return g;
}

// ---- the exact re-score ------------------------------------------------------------------------------------
// the per-group parameter view the exact functions read (hbx_exact_impl.h)
struct GrpView {
  int32_t n;
  const double* bw;
  const int32_t* vartype;
  const int32_t* nlev;
  double prod_bw_c;
};

// KDE kd of group b (one thread): prod(bw[iscontinuous]) sequentially in dim order, the reference's order
__device__ __forceinline__ GrpView grp_view(const GrpModel& M, int64_t b, int kd) {
  GrpView v;
  v.n = (int32_t)(kd ? M.n_bad : M.n_good)[b];
  v.bw = (kd ? M.bw_bad : M.bw_good) + b * M.D;
  v.nlev = (kd ? M.nlev_bad : M.nlev_good) + b * M.D;
  v.vartype = M.vartype;
  double p = 1.0;
  for (int d = 0; d < M.D; ++d) p *= (M.vartype[d] == 0) ? v.bw[d] : 1.0;
  v.prod_bw_c = p;
  return v;
}

#define GRP_SEL_THREADS 256

// The shortlist of one chunk of GRP_SEL_THREADS candidates (thread = candidate, `in`: listed) in index order:
// slist[0 .. tot) = the listed threads; whole block, returns tot.  swc: a counter per wave.
__device__ __forceinline__ int grp_compact(bool in, int32_t* swc, int32_t* slist) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t bal = __ballot(in);
  if (lane == 0) swc[wv] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < GRP_SEL_THREADS / 64; ++w) {
    off += w < wv ? swc[w] : 0;
    tot += swc[w];
  }
  if (in) slist[off + __popcll(bal & ((1ull << lane) - 1))] = tid;
  __syncthreads();
  return tot;
}

// both exact fp64 pdfs of the candidate x in the reference's arithmetic, by the whole block; valid in thread 0
__device__ __forceinline__ void grp_exact_both(const GrpView* vw, int D, const double* x, const double* Xs,
                                               const int64_t* rows_g, const int64_t* rows_b, ExactShared* sh, double* l,
                                               double* g) {
  exact_setup(&vw[0], D, x, sh);
  *l = exact_pdf(Xs, D, rows_g, &vw[0], sh);
  __syncthreads();
  exact_setup(&vw[1], D, x, sh);
  *g = exact_pdf(Xs, D, rows_b, &vw[1], sh);
}

// ---- host checks ------------------------------------------------------------------------------------------
// B * S * C within int32 (what every grid, every slot index, list entry and count relies on)
static inline bool grp_counts_ok(int64_t B, int64_t S, int64_t C) {
  if (B < 0 || S < 0 || C < 0 || B > INT32_MAX || S > INT32_MAX) return false;
  if (S > 0 && B > (int64_t)INT32_MAX / S) return false;
  return !(C > 0 && B * S > (int64_t)INT32_MAX / C);
}

static inline int grp_check_dim(const char* who, int32_t D) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  return HBX_OK;
}

static inline bool grp_model_null(const GrpModel& M) {
  return !M.X || !M.seg_off || !M.order || !M.n_good || !M.n_bad || !M.vartype || !M.bw_good || !M.bw_bad ||
         !M.nlev_good || !M.nlev_bad;
}

// f64 / i64 arrays on 8 bytes, i32 arrays on 4
static inline bool grp_model_misaligned(const GrpModel& M) {
  const uintptr_t a8 = (uintptr_t)M.X | (uintptr_t)M.seg_off | (uintptr_t)M.order | (uintptr_t)M.n_good |
                       (uintptr_t)M.n_bad | (uintptr_t)M.bw_good | (uintptr_t)M.bw_bad;
  const uintptr_t a4 = (uintptr_t)M.vartype | (uintptr_t)M.nlev_good | (uintptr_t)M.nlev_bad;
  return (a8 & 7) || (a4 & 3);
}
