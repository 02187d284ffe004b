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
// (c == 1; h == 0, or h > 0 and finite), a bandwidth is not a positive finite number, or the dims exceed the slot bucket
// picked from D
// (hbx_groups.hip's buckets: D <= 8, 16, 32 any mix; D <= 96 up to 64 continuous + 32 categorical).  Its values are
// ln of the reference's own fp64 pdf: NaN where that is negative or NaN, -inf where it underflows to 0.
//
// The fp32 pass, glp_dd_kernel<DCP, DUP, NW, DT>: built from hbx_groups_impl.h's pieces for one KDE (the slots, the
// row layout, the per-slot constants, grp_stage, grp_load_cand, the pair exponent grp_pair_t and its dispatch -- the
// acquisition's screens use the same ones; this pass keeps its own sums and its own bound) -- lane = candidate
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
#include "hbx_groups_impl.h"

#define GLP_HEAD 256  // workspace header: the four counters (u64) in its first 32 bytes
#define GLP_G 4       // terms per fp32 group
#define GLP_K 40      // pairs more than K log2 units under the largest are bounded, not tracked
#define GLP_BAD (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED)

struct GlpArgs {
  GrpModel M;
  const double* cand;
  int64_t C;
  int32_t tiles;     // ceil(C / 64)
  int32_t kd0;       // first KDE of the launch's grid.y (0: good / ln_l, 1: bad / ln_g)
  int32_t fp64_only;
  double rtol;
  double* out[2];    // ln_l, ln_g (nullable)
  int32_t* status;
  unsigned long long* stat;  // the header's counters
  int32_t* cnt;              // [B][2] listed candidates per (group, KDE)
  int32_t* list;             // [B][2][C]
};

// status[b] from grp_classify's bits (hbx_groups_impl.h), one wave per group.  The ln-pdf's reading of them, stated
// here and nowhere else: HBX_GRP_EXACT_L / _G per KDE where it cannot be screened (GRP_EXACT(kd)) -- and also where a
// match factor is negative (h > 1, GRP_NEG(kd)): the fp32 and fp64 passes sum positive terms only, so a signed KDE
// goes through the exact pdf (the acquisition screens it as a signed sum).  UNSUPPORTED comes alone.
__global__ __launch_bounds__(256) void glp_status_kernel(GlpArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= A.M.B) return;  // whole wave
  int dc, du;
  const int c = grp_classify(A.M, b, &dc, &du);
  int st = 0;
  if (c & GRP_NO_MODEL)
    st = HBX_ACQ_NO_MODEL;
  else if (c & GRP_UNSUPPORTED)
    st = HBX_ACQ_UNSUPPORTED;
  else
    st = ((c & (GRP_EXACT(0) | GRP_NEG(0))) ? HBX_GRP_EXACT_L : 0) | ((c & (GRP_EXACT(1) | GRP_NEG(1))) ? HBX_GRP_EXACT_G : 0);
  if (lane == 0) A.status[b] = st;
}

// One staged chunk's pairs for this lane's candidate: rows[0 .. jmax) of the wave's LDS rows (grp_pair_t's exponent
// from t0 = 0, piece counts as there), GLP_G terms per fp32 group, the groups into S.
template <int DCP, int DUP, int QC, int QU>
__device__ __forceinline__ void glp_pairs(const float* __restrict__ rows, int rs, int jmax, int dcq, int duq,
                                          const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                          float& m, double& S) {
  for (int j0 = 0; j0 < jmax; j0 += GLP_G) {
    float s4 = 0.f;
#pragma unroll
    for (int g = 0; g < GLP_G; ++g) {
      if (j0 + g >= jmax) break;  // uniform
      const float t = grp_pair_t<DCP, DUP, QC, QU, false>((const float4*)(rows + (j0 + g) * rs), dcq, duq, xc, xu, dl,
                                                          nullptr, 0.f, nullptr);
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

// the dispatch's call: this lane's candidate against jmax staged rows, piece counts (QC, QU)
#define GLP_PAIRS_CALL(QC, QU) glp_pairs<DCP, DUP, QC, QU>(wrows, lay.rs, jmax, lay.dcq, lay.duq, xc, xu, dl, m, S)

template <int DCP, int DUP, int NW, int DT>
__global__ __launch_bounds__(64 * NW) void glp_dd_kernel(GlpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  GRP_CONSTS_LDS(K, DCP, DUP, 1);  // the constants of KDE kd alone
  __shared__ uint32_t s_bmax[DCP];
  __shared__ float s_pm[NW][64];
  __shared__ double s_ps[NW][64];
  __shared__ int32_t s_i[2];
  __shared__ double s_norm, s_lbln, s_sdp, s_sad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.M.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  if (st & (GLP_BAD | (kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L))) return;  // uniform: the later kernels write these
  const int64_t i = (int64_t)tile * 64 + lane;
  const bool valid = i < A.C;
  if (wave == 0) {
    int dc, du;
    grp_slots(A.M, lane, K.cdim, K.udim, &dc, &du);  // (dc <= DCP, du <= DUP: the status kernel checked the bucket)
    if (lane == 0) {
      s_i[0] = dc;
      s_i[1] = du;
    }
  }
  __syncthreads();
  const int dc = s_i[0], du = s_i[1];
  const int64_t s0 = A.M.seg_off[b], n = A.M.seg_off[b + 1] - s0;
  const int64_t nk = kd ? A.M.n_bad[b] : A.M.n_good[b];
  const double* Xs = A.M.X + s0 * D;
  const int64_t* rows = A.M.order + s0 + (kd ? n - nk : 0);
  const double* bw = (kd ? A.M.bw_bad : A.M.bw_good) + b * D;
  const int32_t* nlev = (kd ? A.M.nlev_bad : A.M.nlev_good) + b * D;
  const GrpLayout lay = grp_layout<DCP, DUP>(D, dc, du);
  for (int e = tid; e < NT * lay.rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  for (int k = tid; k < DCP; k += NT) s_bmax[k] = 0u;
  grp_consts_fill<NT>(K, A.M, b, kd, dc, du, lay.dc4, tid);  // (1 - h >= 0 here: a negative factor is an EXACT KDE)
  __syncthreads();
  // This pass's own sums, in slot order (deterministic): fp64 and, for lb, in ln units -- the screens' (grp_screen_sums)
  // are the fp32 chain's start and its bound, other quantities
  if (tid == 0) {
    double sl = 0.0, lbln = 0.0, sdp = 0.0, sad = 0.0;
    for (int k = 0; k < dc; ++k) sl += log(bw[K.cdim[k]]);
    for (int u = 0; u < du; ++u) {
      const int d = K.udim[u];
      lbln += log(bw[d] / (double)(nlev[d] - 1));
      if (K.delta[0][u] > -1e29f) {
        sdp += fmax((double)K.delta[0][u], 0.0);
        sad += fabs((double)K.delta[0][u]);
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
  grp_load_cand<DCP, DUP>(x, dc, du, K.cdim, K.udim, K.scale[0], K.mu, K.delta[0], xc, xu, dl, certified);
  float m = -INFINITY;
  double S = 0.0;
  float* wrows = sobs + (size_t)wave * 64 * lay.rs;
  for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * 64) {  // uniform trip count: the barriers are block-wide
    __syncthreads();  // (the rows of the previous round are read)
    const int64_t j0 = c0 + (int64_t)wave * 64;
    const int jmax = (int)(nk - j0 < 64 ? (nk - j0 > 0 ? nk - j0 : 0) : 64);
    if (jmax > 0) grp_stage<16>(Xs, D, rows, j0, jmax, wrows, lay.rs, lay.rpp, dc, K.doff, K.dsc[0], K.dmu, s_bmax, lane);
    __syncthreads();
    if (jmax > 0) GRP_PAIRS_DISPATCH_UNSIGNED(DCP, lay, du == 0 ? 0 : 1, GLP_PAIRS_CALL);
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
  const double L = (double)(lay.dc4 + lay.du4 + 1);
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
  const int D = A.M.D;
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
    grp_slots(A.M, lane, s_cdim, s_udim, &dc, &du);
    if (lane == 0) {
      s_i[0] = dc;
      s_i[1] = du;
    }
  }
  __syncthreads();
  const int dc = s_i[0], du = s_i[1];
  const int64_t s0 = A.M.seg_off[b], n = A.M.seg_off[b + 1] - s0;
  const int64_t nk = kd ? A.M.n_bad[b] : A.M.n_good[b];
  const double* Xs = A.M.X + s0 * D;
  const int64_t* rows = A.M.order + s0 + (kd ? n - nk : 0);
  const double* bw = (kd ? A.M.bw_bad : A.M.bw_good) + b * D;
  const int32_t* nlev = (kd ? A.M.nlev_bad : A.M.nlev_good) + b * D;
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
  __shared__ GrpView vw;
  const int D = A.M.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  if ((st & GLP_BAD) || !(st & (kd ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L))) return;  // uniform
  const int64_t s0 = A.M.seg_off[b], n = A.M.seg_off[b + 1] - s0;
  const int64_t nk = kd ? A.M.n_bad[b] : A.M.n_good[b];
  const double* Xs = A.M.X + s0 * D;
  const int64_t* rows = A.M.order + s0 + (kd ? n - nk : 0);
  if (threadIdx.x == 0) vw = grp_view(A.M, b, kd);
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

static int64_t glp_cnt_bytes(int64_t B) { return (B * 2 * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15; }

extern "C" {

int64_t hbx_kde_logpdf_groups_workspace_bytes(int64_t B, int64_t C, int32_t D) {
  if (D < 1 || D > HBX_MAX_D || !grp_counts_ok(B, 1, C)) return -1;
  return GLP_HEAD + glp_cnt_bytes(B) + B * C * 2 * (int64_t)sizeof(int32_t);
}

int hbx_kde_logpdf_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                          const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad, const double* cand,
                          int64_t C, double rtol, int32_t flags, double* ln_l, double* ln_g, int32_t* status,
                          void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_logpdf_groups";
  if (const int rc = grp_check_dim(who, D)) return rc;
  if (B < 0 || C < 0) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld", who, (long long)B, (long long)C);
  if (!grp_counts_ok(B, 1, C))  // (what every grid, list entry and count relies on)
    return hbx_fail(HBX_ERR_ARG, "%s: B * C = %lld * %lld exceeds int32", who, (long long)B, (long long)C);
  if (!(rtol > 0.0)) return hbx_fail(HBX_ERR_ARG, "%s: rtol=%g must be positive", who, rtol);
  if (flags & ~HBX_LOGPDF_FP64_ONLY) return hbx_fail(HBX_ERR_ARG, "%s: flags=%d", who, flags);
  if (!ln_l && !ln_g) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (ln_l and ln_g)", who);
  if (B == 0 || C == 0) return HBX_OK;
  GlpArgs A;
  A.M = grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad);
  if (grp_model_null(A.M) || !cand || !status || !workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if (grp_model_misaligned(A.M) || (((uintptr_t)cand | (uintptr_t)ln_l | (uintptr_t)ln_g) & 7) ||
      ((uintptr_t)status & 3) || ((uintptr_t)workspace & 15))
    return hbx_fail(HBX_ERR_ARG, "%s: pointers must be aligned (f64 / i64: 8 bytes, i32: 4, workspace: 16)", who);
  const int64_t need = hbx_kde_logpdf_groups_workspace_bytes(B, C, D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  A.cand = cand;
  A.C = C;
  A.tiles = (int32_t)((C + 63) / 64);
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
#define GLP_LAUNCH_DD(DCP, DUP, NW, DT) hipLaunchKernelGGL((glp_dd_kernel<DCP, DUP, NW, DT>), grid, dim3(64 * NW), 0, s, A)
#define GLP_LAUNCH_F64(DCP, DUP, NW, DT) \
  hipLaunchKernelGGL((glp_f64_kernel<DCP, DUP, NW, true>), grid, dim3(64 * NW), 0, s, A)
#define GLP_LAUNCH_F64_EXP32(DCP, DUP, NW, DT) \
  hipLaunchKernelGGL((glp_f64_kernel<DCP, DUP, NW, false>), grid, dim3(64 * NW), 0, s, A)
  if (!A.fp64_only) {
    GRP_BUCKET_LAUNCH(D, GLP_LAUNCH_DD);
    HBX_LAUNCH_CHECK();
  }
  if (rtol < 1e-5)
    GRP_BUCKET_LAUNCH(D, GLP_LAUNCH_F64);
  else
    GRP_BUCKET_LAUNCH(D, GLP_LAUNCH_F64_EXP32);
  HBX_LAUNCH_CHECK();
#undef GLP_LAUNCH_DD
#undef GLP_LAUNCH_F64
#undef GLP_LAUNCH_F64_EXP32
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
