// hbx_groups.hip -- grouped acquisition: one exact pick per KDE pair for B independent brackets in two
// launches (hbx_kde_acquire_groups; bohb.py:124-169 per bracket, after the batched refit bohb.py:220-246), and one
// per get_config request when a bracket issues S of them (hbx_kde_acquire_groups_batch, below).
//
// Inputs are hbx_kde_fit's, as they lie on the device: group b's rows are X[seg_off[b] + order[seg_off[b] + j]],
// good KDE j < n_good[b], bad KDE j in [n - n_bad[b], n); its bandwidths and level counts are bw_*[b][D],
// nlev_*[b][D]; its candidate pool is cand[b][C][D].  No KdeParams, no prepared table, no prepare step, no host
// synchronisation: every per-group constant is derived inside the kernels.
//
// Launch 1, groups_screen_kernel<DCP, DUP, NW, DT>: grid = B x ceil(C / 64) linear in blockIdx.x, NW waves.
//   Lane = candidate (its scaled coordinates in registers), the block's waves take the KDE's 64-observation
//   chunks in turn (wave w: chunks w, w + NW, ...), each staged into the wave's LDS rows as fp32 and read back as
//   broadcasts.  Per pair, in log2 units (fp32, direct differences -- no expansion, so no cancellation):
//     t_ij = lb + sum_c -(a_ic - b_jc)^2 + sum_u m_iju delta_u,      a = fl(s_c (x_c - mu_c)), b = fl(s_c (X_jc - mu_c))
//   s_c = sqrt(log2 e / 2) / h_c, mu_c = mean of the group's first <= 64 good rows (any centre is exact algebra; this
//   one keeps |a|, |b| small), m = [x_u == X_ju], lb = sum_u log2(h_u / (c_u - 1)), delta_u = log2|1 - h_u| - log2(h_u /
//   (c_u - 1)) (-1e30 where 1 - h_u == 0: the term is exactly 0).  A categorical h > 1 makes the match factor negative:
//   the term's sign is the parity of its matches in such dims, and positive and negative terms are summed apart.
//   Running log-sum-exp per lane with an INTEGER running maximum m = max ceil(t): the sums S+-, in units of 2^m,
//   are rescaled by ldexp (exact), each term adds exp2(t - m).  No static offset, no underflow, no rescue pass.
//   The waves' (m, S+, S-) meet in LDS and merge by ldexp.  Output per candidate: KdeEst {ln S+, ln S-, err} per
//   KDE (the normalisation -ln n - sum_c ln(h_c sqrt(2 pi)) added in fp64) -> score_interval() (hbx_acq_impl.h)
//   unchanged -> GScreen {slo, shi, rel, flags} in the workspace.
//   The slot bucket is picked by the host from D alone (vartype is device memory): D <= 8, 16, 32 -> every dim
//   may be of either kind (DCP = DUP = the bucket); D <= 96 -> up to 64 continuous and 32 categorical.  Inside a
//   bucket, dc <= 32 with du <= 8 (config #5: 24c + 8u) runs a loop without branches, its piece counts compile-time
//   (grp_pairs_fast); everything else a loop with a uniform branch per 4-slot piece (grp_pairs).
//   Staging: lane = (row in pass, dim), so a row's D doubles are read by consecutive lanes, 16 passes of loads in
//   flight; the chunk's row positions come in one coalesced load and reach the lanes by a lane exchange.
//
//   Error bound (u = 2^-24), per candidate i and KDE, with A_c = |a_ic|, B_c = max_j |b_jc| (taken while staging),
//   R_c = A_c + B_c:
//     - a and b are fp64 products rounded once: |a - a*| <= u |a*|, |b - b*| <= u |b*| (the fp64 roundings of s, of the
//       subtraction and of the product are 2^-29 of that and sit in the 1.02 below); dd = fl(a - b) adds u |a - b|.
//       So |dd - d*| <= 2.02 u R_c, |dd + d*| <= 2.01 R_c and |dd^2 - d*^2| <= 4.1 u R_c^2.
//     - t is a chain of dc + du fma steps from fl(lb), one rounding each of at most u |partial|, and every partial
//       is bounded by T = |lb| + sum_c R_c^2 + sum_u |delta_u| (finite deltas); fl(lb) and fl(delta_u) add u (|lb| +
//       sum |delta_u|); m is exact (integer codes below 2^24).
//     => |t - t*| <= E_t = 1.02 u (dc + du + 8) T.  A term's weight is off by a factor within 2^+-E_t, and
//       2^E - 1 <= 1.05 E for E <= 0.5; candidates with E_t > 0.5 (or any non-finite coordinate or sum) are not
//       certified and are shortlisted unconditionally.
//     - the sums: rescaling is exact (integer exponents; a flush below 2^-126 is beyond the slack).  A term e =
//       exp2(fl(t - m)): the argument's rounding u |t - m| changes e by at most 0.7 u |t - m| 2^-|t - m| <= 0.372 u,
//       v_exp_f32 by 2 u e; with the largest term in (1/2, 1] the sum is >= 1/2, so n terms add at most (2 + 0.75 n) u
//       relative, their n additions n u, the merge NW more.
//     => err = 1.05 E_t + (2 n + 40) u (32 for the merge and the flushes, 8 for log2 of the sum), relative, per sum,
//       against S+ + S-: exactly what est_interval() expects; its own slack covers the final rounding to float.
//
// Launch 2, groups_select_kernel: one block per group (per request, below).  U = min shi over the certified candidates; the shortlist
//   is {slo <= U} plus the uncertified ones, and of the candidates whose score is certainly exactly 1 (both pdfs
//   certainly below the 1e-8 clamps) only the first index.  Every shortlisted candidate gets both exact fp64 pdfs
//   in the reference's arithmetic (hbx_exact_impl.h: the single path's functions, fed a per-group parameter view),
//   then bohb_score, the strict argmin by (score, index), near_best and the record.  A group is exact-only (every
//   candidate re-scored, HBX_ACQ_OVERFLOW) when a continuous bandwidth is not a positive finite number, a
//   categorical dim has a single level (c == 1, h == 0), the dims exceed the bucket, or a pdf bound leaves fp64's
//   exp range.  Correctness never rests on the screen: it only decides what is re-scored.
//   The exact scores are kept in the candidates' GScreen slots for the near-tie count (no second buffer).
//
// S requests per group (hbx_kde_acquire_groups_batch; bohb.py:124-169 once per get_config call of a stage,
// HB_iteration.py:136-138): cand is [B][S][C][D], request q = b S + s has its own pool, its own record q and its own
// select block (grid B S: screen slots from q C, candidates from q C D; U, the first certain 1, the shortlist, the
// argmin and the near count never leave the request).  The screen is per candidate, so it sees group b's S C
// candidates as one flattened pool P of ceil(S C / 64) tiles (a tile may straddle two requests).  Which screen runs
// is grp_tile_screen()'s rule, in one place: S == 1 is hbx_kde_acquire_groups itself, launch 1 above; from
// GRP_TILES_MIN tiles per group on, the tile screen below; under that, launch 1 over the flattened pool.
//
// The tile screen, groups_tiles_kernel<DCP, DUP, NW, DT>: grid = B x slabs, a block is one group and a slab of NW
//   of its tiles (slabs = ceil(tiles / NW)); wave w owns tile tile0 + w, lane = candidate.  Every wave walks every
//   chunk of a KDE for its own candidates: no partial sums, no merge.  The group's status, slots, centres, scales,
//   lb, deltas and norms are derived once per block and serve the slab's NW tiles.  (Slabs of 2, 4 and 8 tiles per
//   wave -- the rows walked again per tile, the constants shared further -- measured within 0.8 % of one tile per
//   wave either way; the loop over them is not kept.)  The rows of the good, then the bad KDE
//   form one stream of chunks of 32 NW rows;
//   chunk g lives in LDS buffer g & 1, each wave stages 32 of its rows exactly as in launch 1 (gather through
//   `order`, centred, scaled, fp32).  One barrier per chunk: past barrier g, chunk g is complete and chunk g - 1 is
//   read by everyone, so each wave first stages its rows of chunk g + 1 into the other buffer and then runs its
//   candidates against chunk g -- a wave's gather is in flight while the other waves of the SIMD do pairs.  The two
//   buffers together are launch 1's LDS rows.  s_bmax is kept per KDE: every row of a KDE is staged before the last
//   barrier of its walk and the bound is formed after that barrier (the bad KDE's first chunk, staged meanwhile,
//   goes to its own maxima) -- so a candidate's bound does not depend on timing.
//   Error bound: E_t is launch 1's, term for term (same a, b, dd, fma chain, same T with B_c from s_bmax).  The sum:
//   one lane adds the n terms of a KDE in row order into one running (m, S+, S-); rescaling is exact, each term
//   carries 0.372 u + 2 u e, each addition u, so the sum is within (2 + 0.75 n) u + n u <= (2 n + 40) u -- launch 1's
//   allowance with its 32 u for the merge left unused.  err = 1.05 E_t + (2 n + 40) u as above.
//   The screens' sums differ in the last bits (another order of additions), so shortlist / near / rel may differ
//   between them; index, score and the pdfs come from the fp64 re-score and do not.
//
// The k best candidates per group (hbx_kde_acquire_groups_topk): launch 1 as above, then groups_topk_kernel in
// launch 2's place -- the k-th smallest upper bound, the shortlist against it, the same re-score, and the ranking of
// hbx_topk_rank.h (shared with hbx_topk.hip).  Its comment, before the kernel, has the steps and the argument why the
// shortlist holds the whole top-k.
//
// The grouped sampler (hbx_kde_sample_groups) lives in hbx_sample.hip beside the draw functions it shares with
// hbx_kde_sample, so the byte-equality of the draws holds by construction.
//
// Where this departs from the plan it was built to, and why:
//   - a block's waves split the observation chunks between them instead of all reading each chunk: at C = 64 (the
//     reference's num_samples, config #5) a group has one wave of candidates, and sharing chunks would leave three
//     of the four waves without work; larger pools simply take more 64-candidate blocks;
//   - the slot bucket comes from D alone, and the kernel sorts the dims into slots itself: vartype is device memory
//     and reading it on the host would be the synchronisation the call must not make;
//   - C == 0 launches one small kernel: the B empty records have to be written by something (NaN is not a byte fill).
#include "hbx_acq_impl.h"
#include "hbx_exact_impl.h"
#include "hbx_topk_rank.h"

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

#define GRP_NO_MODEL 1
#define GRP_UNSUPPORTED 2
#define GRP_EXACT_ONLY 4
#define GRP_NEG_G 8
#define GRP_NEG_B 16

struct GrpArgs {
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
  int64_t B, S, C;  // groups, requests per group (1: hbx_kde_acquire_groups), candidates per request
  int64_t P;        // S * C: the group's flattened pool, what the screen sees
  int32_t D, tiles;  // tiles = ceil(P / 64)
  int32_t dcp, dup;  // slots of the screen instance launched
  int32_t slabs;     // tile screen: blocks per group, one tile per wave
  GScreen* scr;
  AcqResult* res;
};

// What kind of group b is: hbx_kde_fit's skip rule, hbx_kde_prepare's per-dim rules.  Called by one whole wave
// (lane = dim, 64 dims at a time); every lane returns the same status and counts.
__device__ int grp_status(const GrpArgs& A, int64_t b, int* dc_out, int* du_out) {
  const int64_t n = A.seg_off[b + 1] - A.seg_off[b], ng = A.n_good[b], nb = A.n_bad[b];
  *dc_out = *du_out = 0;
  if (ng <= 0 || ng > n || nb <= 0 || nb > n) return GRP_NO_MODEL;  // (uniform)
  const int lane = threadIdx.x & 63;
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
      const double h = (kd ? A.bw_bad : A.bw_good)[b * A.D + d];
      if (cont) {
        if (!(h > 0.0 && h < INFINITY)) st |= GRP_EXACT_ONLY;  // pdf NaN (or 0) everywhere: the exact path says which
      } else {
        const int c = (kd ? A.nlev_bad : A.nlev_good)[b * A.D + d];
        if (c == 1 && h == 0.0)
          st |= GRP_EXACT_ONLY;  // one observed level: match -> 1, mismatch -> 0 / 0
        else if (c < 2 || !(h > 0.0) || h != h)
          st |= GRP_UNSUPPORTED;  // (c == -1: codes not integers in [0, 1024))
        else if (!(h < INFINITY))
          st |= GRP_EXACT_ONLY;
        else if (1.0 - h < 0.0)
          st |= kd ? GRP_NEG_B : GRP_NEG_G;
      }
    }
  }
  st = (int)wave_reduce_dpp((uint32_t)st, OpOr());
  if (dc > A.dcp || du > A.dup) st |= GRP_EXACT_ONLY;
  *dc_out = dc;
  *du_out = du;
  return st;
}

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

__device__ __forceinline__ float grp_uniform(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// One staged chunk's pairs for this lane's candidate: rows[0 .. jmax) of the wave's LDS rows (stride rs floats:
// continuous slots from 0, categorical slots from 4 dcq).
template <int DCP, int DUP, bool SG>
__device__ __forceinline__ void grp_pairs(const float* __restrict__ rows, int rs, int jmax, int dc, int du, int dcq,
                                          const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                          const float (&nf)[DUP], float lbs, float& m, float& sp, float& sn) {
  for (int j = 0; j < jmax; ++j) {
    const float4* rj = (const float4*)(rows + j * rs);
    float t = lbs, par = 0.f;
#pragma unroll
    for (int q = 0; q < DCP / 4; ++q)
      if (4 * q < dc) {  // uniform
        const float4 v = rj[q];
        const float d0 = xc[4 * q] - v.x, d1 = xc[4 * q + 1] - v.y, d2 = xc[4 * q + 2] - v.z, d3 = xc[4 * q + 3] - v.w;
        t = fmaf(-d0, d0, t);
        t = fmaf(-d1, d1, t);
        t = fmaf(-d2, d2, t);
        t = fmaf(-d3, d3, t);
      }
#pragma unroll
    for (int q = 0; q < DUP / 4; ++q)
      if (4 * q < du) {  // uniform
        const float4 v = rj[dcq + q];
        const float m0 = cat_match(xu[4 * q], v.x), m1 = cat_match(xu[4 * q + 1], v.y);
        const float m2 = cat_match(xu[4 * q + 2], v.z), m3 = cat_match(xu[4 * q + 3], v.w);
        t = fmaf(m0, dl[4 * q], t);
        t = fmaf(m1, dl[4 * q + 1], t);
        t = fmaf(m2, dl[4 * q + 2], t);
        t = fmaf(m3, dl[4 * q + 3], t);
        if (SG) {
          par = fmaf(m0, nf[4 * q], par);
          par = fmaf(m1, nf[4 * q + 1], par);
          par = fmaf(m2, nf[4 * q + 2], par);
          par = fmaf(m3, nf[4 * q + 3], par);
        }
      }
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

// The same without a branch in the loop: QC continuous and QU categorical 4-slot pieces, compile-time counts (the
// padding slots are zeros on both sides: a zero difference, a match with delta 0).  Every LDS read of a row is
// issued before its first use -- with the uniform branches of grp_pairs between them the compiler waits for each
// read on its own, one LDS latency per piece instead of one per pair.
template <int DCP, int DUP, int QC, int QU, bool SG>
__device__ __forceinline__ void grp_pairs_fast(const float* __restrict__ rows, int rs, int jmax,
                                               const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                               const float (&nf)[DUP], float lbs, float& m, float& sp, float& sn) {
  static_assert(4 * QC <= DCP && 4 * QU <= DUP, "pieces within the slots");
  for (int j = 0; j < jmax; ++j) {
    const float4* rj = (const float4*)(rows + j * rs);
    float4 vc[QC > 0 ? QC : 1], vu[QU > 0 ? QU : 1];
#pragma unroll
    for (int q = 0; q < QC; ++q) vc[q] = rj[q];
#pragma unroll
    for (int q = 0; q < QU; ++q) vu[q] = rj[QC + q];
    float t = lbs, par = 0.f;
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
      const float m0 = cat_match(xu[4 * q], v.x), m1 = cat_match(xu[4 * q + 1], v.y);
      const float m2 = cat_match(xu[4 * q + 2], v.z), m3 = cat_match(xu[4 * q + 3], v.w);
      t = fmaf(m0, dl[4 * q], t);
      t = fmaf(m1, dl[4 * q + 1], t);
      t = fmaf(m2, dl[4 * q + 2], t);
      t = fmaf(m3, dl[4 * q + 3], t);
      if (SG) {
        par = fmaf(m0, nf[4 * q], par);
        par = fmaf(m1, nf[4 * q + 1], par);
        par = fmaf(m2, nf[4 * q + 2], par);
        par = fmaf(m3, nf[4 * q + 3], par);
      }
    }
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

// The branch-free instances: up to 32 continuous dims in 2, 4, 6 or 8 pieces and up to 8 categorical dims in 0 or
// 2 pieces (config #5's 24c + 8u: 6 + 2); var = 3 * (QC / 2 - 1) + (no categorical dim ? 0 : signed ? 2 : 1).
// Everything else takes grp_pairs.
template <int DCP, int DUP, int QC>
__device__ __forceinline__ void grp_pairs_qc(int cat, const float* __restrict__ rows, int rs, int jmax,
                                             const float (&xc)[DCP], const float (&xu)[DUP], const float (&dl)[DUP],
                                             const float (&nf)[DUP], float lbs, float& m, float& sp, float& sn) {
  if constexpr (4 * QC <= DCP) {
    if (cat == 0)
      grp_pairs_fast<DCP, DUP, QC, 0, false>(rows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else if (cat == 1)
      grp_pairs_fast<DCP, DUP, QC, 2, false>(rows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else
      grp_pairs_fast<DCP, DUP, QC, 2, true>(rows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
  }
}

template <int DCP, int DUP, int NW, int DT>
__global__ __launch_bounds__(64 * NW) void groups_screen_kernel(GrpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  __shared__ double s_scale[2][DCP], s_mu[DCP], s_lnh[2][DCP], s_lb[2][DUP];
  __shared__ float s_delta[2][DUP], s_negf[2][DUP];
  __shared__ int32_t s_cdim[DCP], s_udim[DUP];
  __shared__ uint32_t s_bmax[DCP];
  __shared__ int32_t s_doff[DCP + DUP];  // dim -> float offset of its slot in a staged row
  __shared__ double s_dsc[2][DCP + DUP], s_dmu[DCP + DUP];  // dim -> scale (categorical: 1) and centre (0)
  __shared__ float s_pm[NW][64], s_ps[NW][64], s_pn[NW][64];
  __shared__ int32_t s_i[4];
  __shared__ double s_norm[2];
  __shared__ float s_lbs[2], s_tfix[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int64_t i = (int64_t)tile * 64 + lane;
  const bool valid = i < A.P;  // (the group's flattened pool: S requests of C candidates)
  GScreen* out = A.scr + b * A.P + i;
  if (wave == 0) {
    int dc, du;
    const int st = grp_status(A, b, &dc, &du);
    if (lane == 0) {
      s_i[0] = st;
      s_i[1] = dc;
      s_i[2] = du;
    }
    if (!(st & (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY))) {  // (then dc <= DCP, du <= DUP): slots in dim order
      int kc = 0, ku = 0;
      for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        const bool cont = d < D && A.vartype[d] == 0, cat = d < D && !cont;
        const uint64_t mc = __ballot(cont), mu = __ballot(cat), below = (1ull << lane) - 1ull;
        if (cont) s_cdim[kc + __popcll(mc & below)] = d;
        if (cat) s_udim[ku + __popcll(mu & below)] = d;
        kc += __popcll(mc);
        ku += __popcll(mu);
      }
    }
  }
  __syncthreads();
  const int st = s_i[0], dc = s_i[1], du = s_i[2];
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY)) {  // no screen: the select kernel re-scores (or skips)
    if (wave == 0 && valid) {
      GScreen g;
      g.slo = g.shi = NAN;
      g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, nullptr) + grp_exact_rel(D, st & GRP_NEG_B, nullptr) + 0x1p-51) *
                      1.000001);
      g.fl = GS_FORCE;
      *out = g;
    }
    return;
  }
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t ng = A.n_good[b], nb = A.n_bad[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* ord = A.order + s0;
  // the row layout: continuous slots from 0, categorical slots from 4 dcq.  Branch-free instances (grp_pairs_fast)
  // serve dc <= 32 in 2 / 4 / 6 / 8 pieces with du <= 8 in 0 / 2 pieces; the rest takes grp_pairs' exact piece counts
  const int qcs = dc <= 8 ? 2 : dc <= 16 ? 4 : dc <= 24 ? 6 : 8;
  const bool fast = dc <= 32 && du <= 8 && 4 * qcs <= DCP;
  const int dcq = fast ? qcs : (dc + 3) >> 2;
  const int dc4 = 4 * dcq, du4 = fast ? (du ? 8 : 0) : (du + 3) & ~3;
  const int rs = dc4 + du4 + 4;  // <= DT + 4
  const int rpp = D <= 64 ? 64 / D : 1;  // rows per staging pass
  for (int e = tid; e < NT * rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  // per-group constants of both KDEs
  for (int k = tid; k < DCP; k += NT) {
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
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) {
        const double h = (kd ? A.bw_bad : A.bw_good)[b * D + d];
        s_scale[kd][k] = sqrt(M_LOG2E / 2.0) / h;
        s_dsc[kd][d] = s_scale[kd][k];
        s_lnh[kd][k] = log(h);
      }
    } else {
      s_mu[k] = 0.0;
      s_scale[0][k] = s_scale[1][k] = 0.0;
    }
  }
  for (int u = tid; u < DUP; u += NT) {
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {
      float dl = 0.f, ngf = 0.f;
      double lb = 0.0;
      if (u < du) {
        const int d = s_udim[u];
        s_doff[d] = dc4 + u;
        s_dsc[kd][d] = 1.0;
        s_dmu[d] = 0.0;
        const double h = (kd ? A.bw_bad : A.bw_good)[b * D + d];
        const int c = (kd ? A.nlev_bad : A.nlev_good)[b * D + d];
        const double a = 1.0 - h;
        lb = log2(h / (double)(c - 1));
        dl = (a == 0.0) ? -1e30f : (float)(log2(fabs(a)) - lb);
        ngf = a < 0.0 ? 1.f : 0.f;
      }
      s_delta[kd][u] = dl;
      s_negf[kd][u] = ngf;
      s_lb[kd][u] = lb;
    }
  }
  __syncthreads();
  if (tid < 2) {  // the sums in slot order (deterministic)
    const int kd = tid;
    double sl = 0.0, lb = 0.0;
    float sad = 0.f;
    for (int k = 0; k < dc; ++k) sl += s_lnh[kd][k];
    for (int u = 0; u < du; ++u) {
      lb += s_lb[kd][u];
      if (s_delta[kd][u] > -1e29f) sad += fabsf(s_delta[kd][u]);
    }
    s_norm[kd] = -log((double)(kd ? nb : ng)) - sl - 0.5 * (double)dc * log(2.0 * M_PI);
    s_lbs[kd] = (float)lb;
    s_tfix[kd] = (fabsf((float)lb) + sad) * 1.0001f;  // |lb| + sum |delta|
  }
  __syncthreads();
  const double* x = A.cand + (b * A.P + (valid ? i : (int64_t)tile * 64)) * D;
  bool certified = true;
  KdeEst est_l = kde_est_neutral(), est_g = kde_est_neutral();
#pragma unroll 1
  for (int kd = 0; kd < 2; ++kd) {
    const int64_t nk = kd ? nb : ng;
    const int64_t* rows = ord + (kd ? n - nb : 0);
    const bool sg = st & (kd ? GRP_NEG_B : GRP_NEG_G);
    float xc[DCP], xu[DUP], dl[DUP], nf[DUP];
#pragma unroll
    for (int k = 0; k < DCP; ++k) {
      xc[k] = 0.f;
      if (k < dc) {
        const double xv = x[s_cdim[k]];
        certified = certified && (xv - xv == 0.0);
        xc[k] = (float)(s_scale[kd][k] * (xv - s_mu[k]));
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
      dl[u] = grp_uniform(s_delta[kd][u]);
      nf[u] = s_negf[kd][u];  // (vector registers: 2 DUP uniform values exceed the scalar file)
    }
    const float lbs = grp_uniform(s_lbs[kd]);
    for (int k = tid; k < DCP; k += NT) s_bmax[k] = 0u;
    float m = -INFINITY, sp = 0.f, sn = 0.f;
    float* wrows = sobs + (size_t)wave * 64 * rs;
    for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * 64) {  // uniform trip count: the barriers are block-wide
      __syncthreads();  // (the rows of the previous round are read; s_bmax zeroed)
      const int64_t j0 = c0 + (int64_t)wave * 64;
      const int jmax = (int)(nk - j0 < 64 ? (nk - j0 > 0 ? nk - j0 : 0) : 64);
      if (jmax > 0) {
        // lane = (row in pass, dim): a row's D doubles are read by consecutive lanes (coalesced), 16 passes of
        // loads in flight; dims past 64 take further rounds (db).  The chunk's row positions come in one coalesced
        // load and reach the lanes by a lane exchange (no dependent global load per pass).
        const int myrow = (int)rows[j0 + (lane < jmax ? lane : 0)];  // (positions local to the segment: < 2^31)
        for (int db = 0; db < D; db += 64) {
          const int lr = D <= 64 ? lane / D : 0;
          const int ld = db + (D <= 64 ? lane - lr * D : lane);
          const bool act = lr < rpp && ld < D;
          const int off = act ? s_doff[ld] : 0;
          const double sc = act ? s_dsc[kd][ld] : 0.0, mu = act ? s_dmu[ld] : 0.0;
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
        const int cat = du == 0 ? 0 : sg ? 2 : 1;
        if (fast && qcs == 2)
          grp_pairs_qc<DCP, DUP, 2>(cat, wrows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
        else if (fast && qcs == 4)
          grp_pairs_qc<DCP, DUP, 4>(cat, wrows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
        else if (fast && qcs == 6)
          grp_pairs_qc<DCP, DUP, 6>(cat, wrows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
        else if (fast)
          grp_pairs_qc<DCP, DUP, 8>(cat, wrows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
        else if (sg)
          grp_pairs<DCP, DUP, true>(wrows, rs, jmax, dc, du, dcq, xc, xu, dl, nf, lbs, m, sp, sn);
        else
          grp_pairs<DCP, DUP, false>(wrows, rs, jmax, dc, du, dcq, xc, xu, dl, nf, lbs, m, sp, sn);
      }
    }
    s_pm[wave][lane] = m;
    s_ps[wave][lane] = sp;
    s_pn[wave][lane] = sn;
    __syncthreads();
    // merge the waves' partials (every wave computes the same numbers for its lane)
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, s_pm[w][lane]);
    float Sp = 0.f, Sn = 0.f;
    bool bad = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float mw = s_pm[w][lane];
      bad = bad || mw != mw;  // (fmaxf drops a NaN)
      if (mw > -INFINITY) {
        const int sh = (int)fmaxf(mw - M, -250.f);
        Sp += ldexpf(s_ps[w][lane], sh);
        Sn += ldexpf(s_pn[w][lane], sh);
      }
    }
    float T = s_tfix[kd];
#pragma unroll
    for (int k = 0; k < DCP; ++k)
      if (k < dc) {
        const float r = fabsf(xc[k]) + __uint_as_float(s_bmax[k]);
        T = fmaf(r, r, T);
      }
    const float u24 = 0x1p-24f;
    const float Et = 1.02f * u24 * (float)(dc + du + 8) * T;
    KdeEst e;
    e.pad = 0.f;
    e.err = 1.05f * Et + (2.f * (float)nk + 40.f) * u24;
    if (!(Et < 0.5f) || bad || !(Sp - Sp == 0.f) || !(Sn - Sn == 0.f) || !(M - M == 0.f)) certified = false;
    const double nrm = s_norm[kd];
    e.lpos = Sp > 0.f ? (float)(((double)__log2f(Sp) + (double)M) * M_LN2 + nrm) : -INFINITY;
    e.lneg = Sn > 0.f ? (float)(((double)__log2f(Sn) + (double)M) * M_LN2 + nrm) : -INFINITY;
    if (kd == 0)
      est_l = e;
    else
      est_g = e;
    __syncthreads();  // (s_pm, s_bmax are rewritten for the bad KDE)
  }
  if (wave != 0 || !valid) return;
  GScreen g;
  if (!certified) {
    g.slo = g.shi = NAN;
    g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, nullptr) + grp_exact_rel(D, st & GRP_NEG_B, nullptr) + 0x1p-51) *
                    1.000001);
    g.fl = GS_FORCE;
  } else {
    const ScoreIv v = score_interval(est_l, est_g);
    g.slo = v.slo;
    g.shi = v.shi;
    g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, &est_l) + grp_exact_rel(D, st & GRP_NEG_B, &est_g) + 0x1p-51) *
                    1.000001);
    g.fl = (v.one ? GS_ONE : 0u) | (v.of ? GS_OF : 0u) | ((v.lnan || v.slo != v.slo || v.shi != v.shi) ? GS_FORCE : 0u);
  }
  *out = g;
}

// The tile screen (header: "The tile screen"): the block is a slab of NW tiles of one group, wave w owns tile
// tile0 + w and walks every chunk of both KDEs itself; the chunks are staged once for the block, 32 NW rows at a
// time in two buffers.  The per-group constants, the staging of a wave's rows, the pair
// loops, the bound and the GScreen are groups_screen_kernel's, statement for statement; they are repeated here and
// not shared, because groups_screen_kernel<32, 32, 4, 40> sits at 255 VGPRs: as one kernel with a compile-time
// switch and the common steps as lambdas it came out at 256 VGPRs + 4 AGPRs, one wave per SIMD instead of two (and
// the 8-slot instance at 174 instead of 165, two waves instead of three).
template <int DCP, int DUP, int NW, int DT>
__global__ __launch_bounds__(64 * NW, DCP <= 32 ? 2 : 1) void groups_tiles_kernel(GrpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  __shared__ double s_scale[2][DCP], s_mu[DCP], s_lnh[2][DCP], s_lb[2][DUP];
  __shared__ float s_delta[2][DUP], s_negf[2][DUP];
  __shared__ int32_t s_cdim[DCP], s_udim[DUP];
  __shared__ uint32_t s_bmax[2][DCP];
  __shared__ int32_t s_doff[DCP + DUP];  // dim -> float offset of its slot in a staged row
  __shared__ double s_dsc[2][DCP + DUP], s_dmu[DCP + DUP];  // dim -> scale (categorical: 1) and centre (0)
  __shared__ int32_t s_i[4];
  __shared__ double s_norm[2];
  __shared__ float s_lbs[2], s_tfix[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.D;
  const int64_t b = (int64_t)blockIdx.x / A.slabs;
  const int tile0 = (int)((int64_t)blockIdx.x - b * A.slabs) * NW;  // the slab's first tile
  if (wave == 0) {
    int dc, du;
    const int st = grp_status(A, b, &dc, &du);
    if (lane == 0) {
      s_i[0] = st;
      s_i[1] = dc;
      s_i[2] = du;
    }
    if (!(st & (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY))) {  // (then dc <= DCP, du <= DUP): slots in dim order
      int kc = 0, ku = 0;
      for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        const bool cont = d < D && A.vartype[d] == 0, cat = d < D && !cont;
        const uint64_t mc = __ballot(cont), mu = __ballot(cat), below = (1ull << lane) - 1ull;
        if (cont) s_cdim[kc + __popcll(mc & below)] = d;
        if (cat) s_udim[ku + __popcll(mu & below)] = d;
        kc += __popcll(mc);
        ku += __popcll(mu);
      }
    }
  }
  __syncthreads();
  const int st = s_i[0], dc = s_i[1], du = s_i[2];
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY)) {  // no screen: the select kernel re-scores (or skips)
    GScreen g;
    g.slo = g.shi = NAN;
    g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, nullptr) + grp_exact_rel(D, st & GRP_NEG_B, nullptr) + 0x1p-51) *
                    1.000001);
    g.fl = GS_FORCE;
    const int64_t iw = (int64_t)(tile0 + wave) * 64 + lane;
    if (iw < A.P) A.scr[b * A.P + iw] = g;
    return;
  }
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t ng = A.n_good[b], nb = A.n_bad[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* ord = A.order + s0;
  // the row layout: continuous slots from 0, categorical slots from 4 dcq.  Branch-free instances (grp_pairs_fast)
  // serve dc <= 32 in 2 / 4 / 6 / 8 pieces with du <= 8 in 0 / 2 pieces; the rest takes grp_pairs' exact piece counts
  const int qcs = dc <= 8 ? 2 : dc <= 16 ? 4 : dc <= 24 ? 6 : 8;
  const bool fast = dc <= 32 && du <= 8 && 4 * qcs <= DCP;
  const int dcq = fast ? qcs : (dc + 3) >> 2;
  const int dc4 = 4 * dcq, du4 = fast ? (du ? 8 : 0) : (du + 3) & ~3;
  const int rs = dc4 + du4 + 4;  // <= DT + 4
  const int rpp = D <= 64 ? 64 / D : 1;  // rows per staging pass
  for (int e = tid; e < NT * rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  for (int k = tid; k < 2 * DCP; k += NT) s_bmax[k / DCP][k % DCP] = 0u;
  // per-group constants of both KDEs
  for (int k = tid; k < DCP; k += NT) {
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
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) {
        const double h = (kd ? A.bw_bad : A.bw_good)[b * D + d];
        s_scale[kd][k] = sqrt(M_LOG2E / 2.0) / h;
        s_dsc[kd][d] = s_scale[kd][k];
        s_lnh[kd][k] = log(h);
      }
    } else {
      s_mu[k] = 0.0;
      s_scale[0][k] = s_scale[1][k] = 0.0;
    }
  }
  for (int u = tid; u < DUP; u += NT) {
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {
      float dl = 0.f, ngf = 0.f;
      double lb = 0.0;
      if (u < du) {
        const int d = s_udim[u];
        s_doff[d] = dc4 + u;
        s_dsc[kd][d] = 1.0;
        s_dmu[d] = 0.0;
        const double h = (kd ? A.bw_bad : A.bw_good)[b * D + d];
        const int c = (kd ? A.nlev_bad : A.nlev_good)[b * D + d];
        const double a = 1.0 - h;
        lb = log2(h / (double)(c - 1));
        dl = (a == 0.0) ? -1e30f : (float)(log2(fabs(a)) - lb);
        ngf = a < 0.0 ? 1.f : 0.f;
      }
      s_delta[kd][u] = dl;
      s_negf[kd][u] = ngf;
      s_lb[kd][u] = lb;
    }
  }
  __syncthreads();
  if (tid < 2) {  // the sums in slot order (deterministic)
    const int kd = tid;
    double sl = 0.0, lb = 0.0;
    float sad = 0.f;
    for (int k = 0; k < dc; ++k) sl += s_lnh[kd][k];
    for (int u = 0; u < du; ++u) {
      lb += s_lb[kd][u];
      if (s_delta[kd][u] > -1e29f) sad += fabsf(s_delta[kd][u]);
    }
    s_norm[kd] = -log((double)(kd ? nb : ng)) - sl - 0.5 * (double)dc * log(2.0 * M_PI);
    s_lbs[kd] = (float)lb;
    s_tfix[kd] = (fabsf((float)lb) + sad) * 1.0001f;  // |lb| + sum |delta|
  }
  __syncthreads();
  // this lane's candidate x against KDE kd: its scaled coordinates, its codes and the KDE's deltas in registers
  auto load_cand = [&](int kd, const double* x, float(&xc)[DCP], float(&xu)[DUP], float(&dl)[DUP], float(&nf)[DUP],
                       bool& certified) {
#pragma unroll
    for (int k = 0; k < DCP; ++k) {
      xc[k] = 0.f;
      if (k < dc) {
        const double xv = x[s_cdim[k]];
        certified = certified && (xv - xv == 0.0);
        xc[k] = (float)(s_scale[kd][k] * (xv - s_mu[k]));
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
      dl[u] = grp_uniform(s_delta[kd][u]);
      nf[u] = s_negf[kd][u];  // (vector registers: 2 DUP uniform values exceed the scalar file)
    }
  };
  // one wave stages rows[j0 .. j0 + jmax) of KDE kd (jmax <= 64) into wrows.  The candidate's registers are live
  // here (the next chunk is staged before this one is read), so the 32-slot instance keeps 8 loads in flight, not 16
  constexpr int SL = DCP >= 32 ? 8 : 16;
  auto stage =[&](int kd, const int64_t* rows, int64_t j0, int jmax, float* wrows) {
    // lane = (row in pass, dim): a row's D doubles are read by consecutive lanes (coalesced), SL passes of
    // loads in flight; dims past 64 take further rounds (db).  The chunk's row positions come in one coalesced
    // load and reach the lanes by a lane exchange (no dependent global load per pass).
    const int myrow = (int)rows[j0 + (lane < jmax ? lane : 0)];  // (positions local to the segment: < 2^31)
    for (int db = 0; db < D; db += 64) {
      const int lr = D <= 64 ? lane / D : 0;
      const int ld = db + (D <= 64 ? lane - lr * D : lane);
      const bool act = lr < rpp && ld < D;
      const int off = act ? s_doff[ld] : 0;
      const double sc = act ? s_dsc[kd][ld] : 0.0, mu = act ? s_dmu[ld] : 0.0;
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
      if (act && off < dc) atomicMax(&s_bmax[kd][off], bm);
    }
  };
  // this lane's candidate against jmax staged rows
  auto pairs = [&](bool sg, const float* srows, int jmax, const float(&xc)[DCP], const float(&xu)[DUP],
                   const float(&dl)[DUP], const float(&nf)[DUP], float lbs, float& m, float& sp, float& sn) {
    const int cat = du == 0 ? 0 : sg ? 2 : 1;
    if (fast && qcs == 2)
      grp_pairs_qc<DCP, DUP, 2>(cat, srows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else if (fast && qcs == 4)
      grp_pairs_qc<DCP, DUP, 4>(cat, srows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else if (fast && qcs == 6)
      grp_pairs_qc<DCP, DUP, 6>(cat, srows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else if (fast)
      grp_pairs_qc<DCP, DUP, 8>(cat, srows, rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    else if (sg)
      grp_pairs<DCP, DUP, true>(srows, rs, jmax, dc, du, dcq, xc, xu, dl, nf, lbs, m, sp, sn);
    else
      grp_pairs<DCP, DUP, false>(srows, rs, jmax, dc, du, dcq, xc, xu, dl, nf, lbs, m, sp, sn);
  };
  // the candidate's sums over KDE kd's nk rows (in units of 2^M) -> KdeEst with the header's bound
  auto estimate = [&](int kd, int64_t nk, const float(&xc)[DCP], float M, float Sp, float Sn, bool bad,
                      bool& certified) {
    float T = s_tfix[kd];
#pragma unroll
    for (int k = 0; k < DCP; ++k)
      if (k < dc) {
        const float r = fabsf(xc[k]) + __uint_as_float(s_bmax[kd][k]);
        T = fmaf(r, r, T);
      }
    const float u24 = 0x1p-24f;
    const float Et = 1.02f * u24 * (float)(dc + du + 8) * T;
    KdeEst e;
    e.pad = 0.f;
    e.err = 1.05f * Et + (2.f * (float)nk + 40.f) * u24;
    if (!(Et < 0.5f) || bad || !(Sp - Sp == 0.f) || !(Sn - Sn == 0.f) || !(M - M == 0.f)) certified = false;
    const double nrm = s_norm[kd];
    e.lpos = Sp > 0.f ? (float)(((double)__log2f(Sp) + (double)M) * M_LN2 + nrm) : -INFINITY;
    e.lneg = Sn > 0.f ? (float)(((double)__log2f(Sn) + (double)M) * M_LN2 + nrm) : -INFINITY;
    return e;
  };
  auto emit = [&](GScreen* out, bool certified, const KdeEst& est_l, const KdeEst& est_g) {
    GScreen g;
    if (!certified) {
      g.slo = g.shi = NAN;
      g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, nullptr) + grp_exact_rel(D, st & GRP_NEG_B, nullptr) + 0x1p-51) *
                      1.000001);
      g.fl = GS_FORCE;
    } else {
      const ScoreIv v = score_interval(est_l, est_g);
      g.slo = v.slo;
      g.shi = v.shi;
      g.rel = (float)((grp_exact_rel(D, st & GRP_NEG_G, &est_l) + grp_exact_rel(D, st & GRP_NEG_B, &est_g) + 0x1p-51) *
                      1.000001);
      g.fl = (v.one ? GS_ONE : 0u) | (v.of ? GS_OF : 0u) | ((v.lnan || v.slo != v.slo || v.shi != v.shi) ? GS_FORCE : 0u);
    }
    *out = g;
  };
  // The rows of the good, then the bad KDE as one stream of chunks of CH = 32 NW rows: chunk g lies in buffer
  // g & 1, every wave stages 32 of its rows.  One barrier per chunk: past it chunk g is staged and chunk g - 1 is
  // read by every wave, so the waves stage chunk g + 1 into the other buffer and then read chunk g -- a wave's
  // gather of the next chunk overlaps the other waves' pairs of this one.
  constexpr int CW = 32, CH = CW * NW;
  auto stage_chunk = [&](int kd, int64_t c, int buf) {
    const int64_t nk = kd ? nb : ng, j0 = c * CH + (int64_t)wave * CW;
    const int jmax = (int)(nk - j0 < CW ? (nk - j0 > 0 ? nk - j0 : 0) : CW);
    if (jmax > 0) stage(kd, ord + (kd ? n - nb : 0), j0, jmax, sobs + ((size_t)buf * CH + (size_t)wave * CW) * rs);
  };
  __syncthreads();  // (s_bmax and the padding slots are zeroed)
  stage_chunk(0, 0, 0);
  int g = 0;
  bool certified = true;
  KdeEst est_l = kde_est_neutral();
  const int tw = tile0 + wave;  // this wave's tile
  const int64_t iw = (int64_t)tw * 64 + lane;
  const bool vw = iw < A.P;
  const bool live = tw < A.tiles;  // (wave-uniform; a wave without a tile still stages its rows)
  const double* x = A.cand + (b * A.P + (vw ? iw : live ? (int64_t)tw * 64 : 0)) * D;
#pragma unroll 1
  for (int kd = 0; kd < 2; ++kd) {
    const int64_t nk = kd ? nb : ng;
    const bool sg = st & (kd ? GRP_NEG_B : GRP_NEG_G);
    float xc[DCP], xu[DUP], dl[DUP], nf[DUP];
    load_cand(kd, x, xc, xu, dl, nf, certified);
    const float lbs = grp_uniform(s_lbs[kd]);
    float m = -INFINITY, sp = 0.f, sn = 0.f;
    const int64_t nch = (nk + CH - 1) / CH;
    for (int64_t c = 0; c < nch; ++c, ++g) {  // uniform trip counts: the barriers are block-wide
      __syncthreads();
      if (c + 1 < nch)
        stage_chunk(kd, c + 1, (g + 1) & 1);
      else if (kd == 0)
        stage_chunk(1, 0, (g + 1) & 1);
      const int jmax = (int)(nk - c * CH < CH ? nk - c * CH : CH);
      if (live) pairs(sg, sobs + (size_t)(g & 1) * CH * rs, jmax, xc, xu, dl, nf, lbs, m, sp, sn);
    }
    // (every row of KDE kd was staged before the walk's last barrier: s_bmax[kd] is complete)
    const KdeEst e = estimate(kd, nk, xc, m, sp, sn, m != m, certified);
    if (kd == 0)
      est_l = e;
    else if (vw)
      emit(A.scr + b * A.P + iw, certified, est_l, e);
  }
}

// the per-group parameter view the exact functions read (hbx_exact_impl.h)
struct GrpView {
  int32_t n;
  const double* bw;
  const int32_t* vartype;
  const int32_t* nlev;
  double prod_bw_c;
};

__device__ __forceinline__ AcqResult grp_empty_record(int32_t flags) {
  AcqResult r;
  r.index = -1;
  r.score = r.pdf_l = r.pdf_g = NAN;
  r.rel = 0.f;
  r.flags = flags;
  r.shortlist = 0;
  r.near = 0;
  return r;
}

#define GRP_SEL_THREADS 256
__global__ __launch_bounds__(GRP_SEL_THREADS) void groups_select_kernel(GrpArgs A) {
  __shared__ ExactShared sh;
  __shared__ GrpView vw[2];
  __shared__ int32_t slist[GRP_SEL_THREADS];
  __shared__ int32_t swc[GRP_SEL_THREADS / 64];
  __shared__ uint32_t s_U;
  __shared__ int32_t s_st, s_of, s_first1, s_none, s_near;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t q = blockIdx.x, b = q / A.S;  // request q = b S + s of group b
  const int D = A.D;
  const int64_t C = A.C;
  if (wv == 0) {
    int dc, du;
    const int st0 = grp_status(A, b, &dc, &du);
    if (lane == 0) s_st = st0;
  }
  if (tid == 0) {
    s_U = hbx_f2ord(INFINITY);
    s_of = 0;
    s_first1 = INT32_MAX;
    s_none = 0;
    s_near = 0;
  }
  __syncthreads();
  const int st = s_st;
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED)) {
    if (tid == 0) A.res[q] = grp_empty_record((st & GRP_NO_MODEL) ? HBX_ACQ_NO_MODEL : HBX_ACQ_UNSUPPORTED);
    return;
  }
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t ng = A.n_good[b], nb = A.n_bad[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* rows_g = A.order + s0;
  const int64_t* rows_b = A.order + s0 + (n - nb);
  if (tid < 2) {  // prod(bw[iscontinuous]) sequentially in dim order: the reference's order
    GrpView v;
    v.n = (int32_t)(tid ? nb : ng);
    v.bw = (tid ? A.bw_bad : A.bw_good) + b * D;
    v.nlev = (tid ? A.nlev_bad : A.nlev_good) + b * D;
    v.vartype = A.vartype;
    double p = 1.0;
    for (int d = 0; d < D; ++d) p *= (A.vartype[d] == 0) ? v.bw[d] : 1.0;
    v.prod_bw_c = p;
    vw[tid] = v;
  }
  GScreen* scr = A.scr + q * C;
  const double* cand = A.cand + q * C * D;
  // pass 1: U = min shi over the certified candidates, the overflow rule, the first certain score 1
  {
    uint32_t u = hbx_f2ord(INFINITY);
    int of = 0, f1 = INT32_MAX, n1 = 0;
    for (int64_t i = tid; i < C; i += GRP_SEL_THREADS) {
      const GScreen g = scr[i];
      if (g.fl & GS_FORCE) continue;
      u = min(u, hbx_f2ord(g.shi));
      of |= (g.fl & GS_OF) ? 1 : 0;
      if (g.fl & GS_ONE) {
        f1 = min(f1, (int)i);
        ++n1;
      }
    }
    atomicMin(&s_U, u);
    if (of) atomicOr(&s_of, 1);
    if (n1) {
      atomicMin(&s_first1, f1);
      atomicAdd(&s_none, n1);
    }
  }
  __syncthreads();
  const bool all = (st & GRP_EXACT_ONLY) || s_of;
  const float U = hbx_ord2f(s_U);
  const int32_t first1 = s_first1;
  // pass 2: the shortlist in index order, 256 candidates at a time; each entry's exact pdfs by the whole block
  double best = INFINITY, bl = NAN, bg = NAN;
  int64_t bidx = -1;
  int32_t nshort = 0;
  for (int64_t c0 = 0; c0 < C; c0 += GRP_SEL_THREADS) {
    const int64_t i = c0 + tid;
    bool in = false;
    if (i < C) {
      const GScreen g = scr[i];
      in = all || (g.fl & GS_FORCE) || ((g.fl & GS_ONE) ? (int32_t)i == first1 : g.slo <= U);
    }
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
    for (int p = 0; p < tot; ++p) {
      const int64_t ip = c0 + slist[p];
      exact_setup(&vw[0], D, cand + ip * D, &sh);
      const double l = exact_pdf(Xs, D, rows_g, &vw[0], &sh);
      __syncthreads();
      exact_setup(&vw[1], D, cand + ip * D, &sh);
      const double g = exact_pdf(Xs, D, rows_b, &vw[1], &sh);
      if (tid == 0) {
        const double s = bohb_score(g, l);
        scr[ip].score = s;
        scr[ip].fl |= GS_DONE;
        if (s < best) {  // index order: strict '<' keeps the first index (bohb.py:149-152; NaN never wins)
          best = s;
          bidx = ip;
          bl = l;
          bg = g;
        }
      }
      __syncthreads();
    }
    nshort += tot;
  }
  // the near set: every re-scored candidate the winner cannot be told apart from by the bounds
  __shared__ double s_best, s_rb;
  __shared__ int64_t s_bidx;
  if (tid == 0) {
    s_best = best;
    s_bidx = bidx;
    s_rb = bidx >= 0 ? (double)scr[bidx].rel : 0.0;
  }
  __threadfence_block();
  __syncthreads();  // (also: thread 0's stores to scr are visible to the block)
  const double sb = s_best, rb = s_rb;
  const int64_t wi = s_bidx;
  if (wi >= 0) {
    int cnt = 0;
    for (int64_t i = tid; i < C; i += GRP_SEL_THREADS) {
      const GScreen g = scr[i];
      if (!(g.fl & GS_DONE)) continue;
      const double s = g.score;
      if (i == wi || near_best(s, (double)g.rel, sb, rb)) ++cnt;
    }
    if (cnt) atomicAdd(&s_near, cnt);
  }
  __syncthreads();
  if (tid == 0) {
    AcqResult r = grp_empty_record(all ? HBX_ACQ_OVERFLOW : 0);
    r.shortlist = nshort;
    int near = s_near;
    // the candidates left out as certain exact 1s tie with a winner whose score is 1
    if (wi >= 0 && !all && sb == 1.0 && s_none > 1) near += s_none - 1;
    r.near = near;
    r.rel = (float)rb;
    if (near > 1) r.flags |= HBX_ACQ_NEAR_TIE;
    if (wi >= 0) {
      r.index = wi;
      r.score = sb;
      r.pdf_l = bl;
      r.pdf_g = bg;
    }
    A.res[q] = r;
  }
}

__global__ void groups_empty_kernel(AcqResult* res, int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) res[b] = grp_empty_record(0);
}

// ------------------------------------------------------------------------------------------
// Grouped top-k (hbx_kde_acquire_groups_topk): the k best candidates of every group's pool, ranked exactly.
// Launch 1 is groups_screen_kernel as hbx_kde_acquire_groups launches it; launch 2 is groups_topk_kernel, one block
// per group, in place of groups_select_kernel:
//   bound      U_k = the k-th smallest shi over the certified candidates (no GS_FORCE; a GS_ONE candidate counts
//              with its interval [0, 0]); fewer than k of them: +inf.  A radix select over the hbx_f2ord keys' four
//              8-bit digits from the top: per digit an LDS histogram of the keys matching the digits chosen so far
//              (the group's slots re-read, so any C), a scan over its 256 bins, the digit that holds the rank.  Counts
//              are integers: no dependence on thread timing.
//   shortlist  in index order, 256 candidates at a time: everything if the group is exact-only or a GS_OF is
//              present; every GS_FORCE candidate; every certified candidate that is not GS_ONE with slo <= U_k; and,
//              only when 0 <= U_k, the first k GS_ONE candidates by index.
//   re-score   both fp64 pdfs of every shortlisted candidate by the whole block (exact_setup / exact_pdf, driven as
//              groups_select_kernel drives them), then bohb_score; the pdfs go to the group's spill in the workspace.
//   ranking    the running best-(k+1) of hbx_topk_rank.h over (score bits, index, index); its LDS arrays are the
//              launch's dynamic LDS, sized from k (grp_topk_cap), beside ExactShared.  An entry's pdfs and rel are not
//              carried through the merges: they stay in the spill / the screen slot and are read by index at the end.
//   result     header and records by ordinary vector stores; HBX_ACQ_NEAR_TIE as the single top-k sets it (adjacent
//              returned entries; the last one and the best re-scored one left out), and also when the last returned
//              entry scores exactly 1 while certain exact-1 candidates were left unlisted.
//
// Why the shortlist holds the whole top-k.  Every certified candidate's true ln score lies in its [slo, shi]; a
// GS_ONE candidate's true score is exactly 1 (ln 0).  With k certified candidates, at least k have shi <= U_k, so at
// least k true scores are <= U_k and the k-th smallest true score is <= U_k: every member of the true top-k, ties by
// index included, has a true score <= U_k, hence slo <= U_k -- or is uncertified, and those are all listed.  (Fewer
// than k certified: U_k = +inf, everything certified passes.)  The added step, for the certain exact 1s: they all
// have the same exact score, so among themselves they rank by index.  One that is preceded by k others of lower
// index is preceded by k candidates of a score not above its own and a lower index, so it cannot be among the first
// k of the order by (score, index): only the first k by index can be returned, and with U_k < 0 none can (k true
// scores are below 1).  The ranking itself is over exact scores only, so the shortlist decides cost, never the
// result.
struct GrpTopk {
  char* out;     // B result blocks of 16 + 40 k bytes
  double2* pdf;  // [B][C] {pdf_l, pdf_g} of the re-scored candidates: the per-group spill
  int32_t k, cap;
};

// entries of the ranking's LDS arrays for k: a power of two with k + 1 + GRP_SEL_THREADS <= cap
static int grp_topk_cap(int32_t k) {
  const int need = k + 1 + GRP_SEL_THREADS;
  return need <= 512 ? 512 : need <= 1024 ? 1024 : 2048;
}
static_assert(HBX_TOPK_MAX_K + 1 + GRP_SEL_THREADS <= 2048, "a chunk fits behind the kept entries after a merge");

__global__ __launch_bounds__(GRP_SEL_THREADS) void groups_topk_kernel(GrpArgs A, GrpTopk K) {
  constexpr int T = GRP_SEL_THREADS;
  extern __shared__ __align__(16) unsigned char s_dyn[];  // the ranking's arrays: cap x (u64, i32, i32)
  __shared__ ExactShared sh;
  __shared__ GrpView vw[2];
  __shared__ int32_t slist[T];
  __shared__ double s_l[T], s_g[T];
  __shared__ int32_t swc[T / 64], swo[T / 64];
  __shared__ uint32_t s_hist[256], s_wsum[T / 64];
  __shared__ uint32_t s_prefix, s_rank;
  __shared__ int32_t s_st, s_of, s_ncert, s_none;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const int D = A.D;
  const int64_t C = A.C;
  const int32_t k = K.k;
  TopkHead* head = (TopkHead*)(K.out + b * (int64_t)(sizeof(TopkHead) + sizeof(TopkRec) * (size_t)k));
  TopkRec* rec = (TopkRec*)(head + 1);
  if (wv == 0) {
    int dc, du;
    const int st0 = grp_status(A, b, &dc, &du);
    if (lane == 0) s_st = st0;
  }
  if (tid == 0) {
    s_of = 0;
    s_ncert = 0;
    s_none = 0;
    s_prefix = 0u;
    s_rank = (uint32_t)k;
  }
  __syncthreads();
  const int st = s_st;
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED)) {
    if (tid == 0) *head = TopkHead{0, 0, (st & GRP_NO_MODEL) ? HBX_ACQ_NO_MODEL : HBX_ACQ_UNSUPPORTED, k};
    return;
  }
  const int64_t s0 = A.seg_off[b], n = A.seg_off[b + 1] - s0;
  const int64_t ng = A.n_good[b], nb = A.n_bad[b];
  const double* Xs = A.X + s0 * D;
  const int64_t* rows_g = A.order + s0;
  const int64_t* rows_b = A.order + s0 + (n - nb);
  if (tid < 2) {  // prod(bw[iscontinuous]) sequentially in dim order: the reference's order
    GrpView v;
    v.n = (int32_t)(tid ? nb : ng);
    v.bw = (tid ? A.bw_bad : A.bw_good) + b * D;
    v.nlev = (tid ? A.nlev_bad : A.nlev_good) + b * D;
    v.vartype = A.vartype;
    double p = 1.0;
    for (int d = 0; d < D; ++d) p *= (A.vartype[d] == 0) ? v.bw[d] : 1.0;
    v.prod_bw_c = p;
    vw[tid] = v;
  }
  const GScreen* scr = A.scr + b * C;
  const double* cand = A.cand + b * C * D;
  double2* pdf = K.pdf + b * C;
  // pass 1: the certified candidates, the certain 1s among them, the overflow rule
  {
    int of = 0, nc = 0, n1 = 0;
    for (int64_t i = tid; i < C; i += T) {
      const uint32_t fl = scr[i].fl;
      if (fl & GS_FORCE) continue;
      ++nc;
      of |= (fl & GS_OF) ? 1 : 0;
      n1 += (fl & GS_ONE) ? 1 : 0;
    }
    if (of) atomicOr(&s_of, 1);
    if (nc) atomicAdd(&s_ncert, nc);
    if (n1) atomicAdd(&s_none, n1);
  }
  __syncthreads();
  const bool all = (st & GRP_EXACT_ONLY) || s_of;
  const int32_t none = s_none;
  // the bound: U_k by radix select over the keys of shi, the top digit first
  float U = INFINITY;
  if (!all && s_ncert >= k) {  // uniform
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
      s_hist[tid] = 0u;  // (T == 256 bins)
      __syncthreads();
      const uint32_t prefix = s_prefix, rank = s_rank;
      for (int64_t i = tid; i < C; i += T) {
        const GScreen g = scr[i];
        if (g.fl & GS_FORCE) continue;
        const uint32_t key = hbx_f2ord(g.shi);
        if (((key ^ prefix) & himask) == 0) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      const uint32_t c = s_hist[tid];
      uint32_t incl = c;  // inclusive scan over the 256 bins: within the wave, then the waves before
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      if (lane == 63) s_wsum[wv] = incl;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < T / 64; ++w) incl += w < wv ? s_wsum[w] : 0u;
      const uint32_t excl = incl - c;
      if (excl < rank && rank <= incl) {  // exactly one bin: the matching keys number >= rank
        s_prefix = prefix | ((uint32_t)tid << shift);
        s_rank = rank - excl;
      }
      __syncthreads();
    }
    U = hbx_ord2f(s_prefix);
  }
  static_assert(T == 256, "one thread per histogram bin");
  TopkRank<T> rank;
  rank.init((uint64_t*)s_dyn, (int32_t*)(s_dyn + 8 * (size_t)K.cap), (int32_t*)(s_dyn + 12 * (size_t)K.cap), swc, K.cap,
            k + 1);  // the k best and the best excluded one (the near-tie test's last pair)
  // pass 2: the shortlist in index order, 256 candidates at a time; each entry's exact pdfs by the whole block
  const bool ones_in = U >= 0.f;
  int32_t nshort = 0, ones_seen = 0;
  for (int64_t c0 = 0; c0 < C; c0 += T) {
    const int64_t i = c0 + tid;
    GScreen g;
    g.fl = GS_FORCE;
    g.slo = g.shi = NAN;
    const bool live = i < C;
    if (live) g = scr[i];
    const bool one = live && !(g.fl & GS_FORCE) && (g.fl & GS_ONE);
    const uint64_t bo = __ballot(one);
    if (lane == 0) swo[wv] = __popcll(bo);
    __syncthreads();
    int obefore = ones_seen, otot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
      obefore += w < wv ? swo[w] : 0;
      otot += swo[w];
    }
    ones_seen += otot;
    bool in = false;
    if (live) {
      if (all || (g.fl & GS_FORCE))
        in = true;
      else if (one)
        in = ones_in && obefore + (int)__popcll(bo & ((1ull << lane) - 1)) < k;  // the first k certain 1s by index
      else
        in = g.slo <= U;
    }
    const uint64_t bal = __ballot(in);
    if (lane == 0) swc[wv] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
      off += w < wv ? swc[w] : 0;
      tot += swc[w];
    }
    if (in) slist[off + __popcll(bal & ((1ull << lane) - 1))] = tid;
    __syncthreads();
    for (int p = 0; p < tot; ++p) {
      const int64_t ip = c0 + slist[p];
      exact_setup(&vw[0], D, cand + ip * D, &sh);
      const double l = exact_pdf(Xs, D, rows_g, &vw[0], &sh);
      __syncthreads();
      exact_setup(&vw[1], D, cand + ip * D, &sh);
      const double gd = exact_pdf(Xs, D, rows_b, &vw[1], &sh);
      if (tid == 0) {
        s_l[p] = l;
        s_g[p] = gd;
      }
      __syncthreads();
    }
    // the chunk's re-scored entries, one per thread in index order: pdfs to the spill, the score to the ranking
    bool acc = false;
    uint64_t key = 0;
    int32_t idx = 0;
    if (tid < tot) {
      const double l = s_l[tid], gd = s_g[tid];
      idx = (int32_t)(c0 + slist[tid]);
      pdf[idx] = make_double2(l, gd);
      const double s = bohb_score(gd, l);
      if (s == s) {  // NaN scores are never returned
        key = (uint64_t)__double_as_longlong(s);
        acc = rank.enters(key, idx);
      }
    }
    rank.push(acc, key, idx, idx);  // (its last barrier: slist, s_l, s_g are free again)
    nshort += tot;
  }
  rank.finish();
  __threadfence_block();
  __syncthreads();  // (the spill's stores are visible to the block)
  const int nbest = rank.nb;
  const int nout = nbest < k ? nbest : k;
  // the ranked records; HBX_ACQ_NEAR_TIE: an entry and the next one (the last returned one's next is the best
  // excluded entry, position k) cannot be told apart by the re-score's error bounds
  bool near = false;
  for (int j = tid; j < nout; j += T) {
    const int32_t idx = rank.si[j];
    const double s = __longlong_as_double((long long)rank.sk[j]);
    const float r = scr[idx].rel;
    const double2 lg = pdf[idx];
    TopkRec o;
    o.index = idx;
    o.score = s;
    o.pdf_l = lg.x;
    o.pdf_g = lg.y;
    o.rel = r;
    o.pad = 0;
    rec[j] = o;
    if (j + 1 < nbest) {
      const double s2 = __longlong_as_double((long long)rank.sk[j + 1]);
      near = near || near_best(s2, (double)scr[rank.si[j + 1]].rel, s, (double)r);
    }
    // the certain 1s left unlisted tie with a last returned entry whose score is 1
    if (j == nout - 1 && s == 1.0 && !all && none > (ones_in ? (none < k ? none : k) : 0)) near = true;
  }
  const int any_near = __syncthreads_or(near);
  if (tid == 0)
    *head = TopkHead{nout, nshort, (all ? HBX_ACQ_OVERFLOW : 0) | (any_near ? HBX_ACQ_NEAR_TIE : 0), k};
}

__global__ void groups_topk_empty_kernel(char* out, int64_t B, int32_t k) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) *(TopkHead*)(out + b * (int64_t)(sizeof(TopkHead) + sizeof(TopkRec) * (size_t)k)) = TopkHead{0, 0, 0, k};
}

#define GRP_WS_HEAD 256

// B * S * C within int32 (what every grid and every screen slot index relies on)
static bool grp_counts_ok(int64_t B, int64_t S, int64_t C) {
  if (B < 0 || S < 0 || C < 0 || B > INT32_MAX || S > INT32_MAX) return false;
  if (S > 0 && B > (int64_t)INT32_MAX / S) return false;
  return !(C > 0 && B * S > (int64_t)INT32_MAX / C);
}

// Which screen a call runs -- the one rule.  One request per group is hbx_kde_acquire_groups' own case: the
// chunk-splitting screen, always.  Several requests flatten to tiles = ceil(S C / 64) tiles per group: from
// GRP_TILES_MIN tiles on the tile screen runs, below that the chunk-splitting screen over the flattened pool.
// Measured at config #5's shape: 2 tiles 10.7 ms against 9.1 ms for the chunk-splitting screen,
// 3 tiles 12.1 against 13.3 (one of the four waves without a tile, and still ahead), 4 tiles 13.7 against 17.7.
// HBX_GROUPS_SCREEN = 1 / 2 forces the chunk-splitting / the tile screen for S > 1 (tests, A/B); read on every call
// like the other switches.
#define GRP_TILES_MIN 3
static bool grp_tile_screen(int64_t S, int64_t tiles) {
  if (S == 1) return false;
  const char* e = getenv("HBX_GROUPS_SCREEN");
  const int v = e ? atoi(e) : 0;
  if (v == 1 || v == 2) return v == 2;
  return tiles >= GRP_TILES_MIN;
}

// One screen launch: the slot bucket from D alone (vartype is on the device), up to D <= 32 any mix of kinds fits
template <bool TILES>
static void grp_launch_screen(GrpArgs& A, hipStream_t s) {
  const int nw = A.D <= 32 ? 4 : 2;  // waves of the bucket's instance
  A.slabs = (A.tiles + nw - 1) / nw;  // the tile screen: one tile per wave
  const dim3 grid((unsigned)(A.B * (TILES ? A.slabs : A.tiles)));  // <= B * S * C <= INT32_MAX
#define GRP_LAUNCH(DCP, DUP, NW, DT)                                                                          \
  do {                                                                                                        \
    A.dcp = DCP;                                                                                              \
    A.dup = DUP;                                                                                              \
    if (TILES)                                                                                                \
      hipLaunchKernelGGL((groups_tiles_kernel<DCP, DUP, NW, DT>), grid, dim3(64 * NW), 0, s, A);              \
    else                                                                                                      \
      hipLaunchKernelGGL((groups_screen_kernel<DCP, DUP, NW, DT>), grid, dim3(64 * NW), 0, s, A);             \
  } while (0)
  if (A.D <= 8)
    GRP_LAUNCH(8, 8, 4, 16);
  else if (A.D <= 16)
    GRP_LAUNCH(16, 16, 4, 24);
  else if (A.D <= 32)
    GRP_LAUNCH(32, 32, 4, 40);
  else  // D <= 96 with <= 64 continuous and <= 32 categorical dims; anything larger is exact-only
    GRP_LAUNCH(64, 32, 2, 104);
#undef GRP_LAUNCH
}

// the argument block of one call: the model, the pools, the screen slots behind the workspace's head
static GrpArgs grp_args(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                        const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                        const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad, const double* cand,
                        int64_t S, int64_t C, void* results, void* workspace) {
  GrpArgs A;
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
  A.S = S;
  A.C = C;
  A.P = S * C;
  A.D = D;
  A.tiles = (int32_t)((A.P + 63) / 64);
  A.scr = (GScreen*)((char*)workspace + GRP_WS_HEAD);
  A.res = (AcqResult*)results;
  return A;
}

// hbx_kde_acquire_groups (S = 1) and hbx_kde_acquire_groups_batch: the checks, the screen, the select
static int grp_acquire(const char* who, const double* X, int32_t D, const int64_t* seg_off, int64_t B,
                       const int64_t* order, const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                       const double* bw_good, const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad,
                       const double* cand, int64_t S, int64_t C, void* results, void* workspace, int64_t ws_bytes,
                       void* stream) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || S < 0 || C < 0)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld S=%lld C=%lld", who, (long long)B, (long long)S, (long long)C);
  if (!grp_counts_ok(B, S, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * S * C = %lld * %lld * %lld exceeds int32", who, (long long)B, (long long)S,
                    (long long)C);
  if (B == 0 || S == 0) return HBX_OK;
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (results)", who);
  hipStream_t s = (hipStream_t)stream;
  if (C == 0) {  // nothing to score: every record is the empty one
    hipLaunchKernelGGL(groups_empty_kernel, dim3((unsigned)((B * S + 255) / 256)), dim3(256), 0, s, (AcqResult*)results,
                       B * S);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !bw_good || !bw_bad || !nlev_good || !nlev_bad ||
      !cand || !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const int64_t need = hbx_kde_groups_batch_workspace_bytes(B, S, C, D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  if (((uintptr_t)workspace & 15) || ((uintptr_t)results & 7))
    return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte, results 8-byte aligned", who);
  GrpArgs A = grp_args(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad, cand, S,
                       C, results, workspace);
  if (grp_tile_screen(S, A.tiles))
    grp_launch_screen<true>(A, s);
  else
    grp_launch_screen<false>(A, s);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(groups_select_kernel, dim3((unsigned)(B * S)), dim3(GRP_SEL_THREADS), 0, s, A);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// hbx_kde_acquire_groups_topk: grp_acquire's checks with S = 1, the same screen, groups_topk_kernel as the select
static int grp_acquire_topk(const char* who, const double* X, int32_t D, const int64_t* seg_off, int64_t B,
                            const int64_t* order, const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                            const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                            const int32_t* nlev_bad, const double* cand, int64_t C, int32_t k, void* results,
                            void* workspace, int64_t ws_bytes, void* stream) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || C < 0) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld", who, (long long)B, (long long)C);
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, HBX_TOPK_MAX_K);
  if (!grp_counts_ok(B, 1, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * C = %lld * %lld exceeds int32", who, (long long)B, (long long)C);
  if (B == 0) return HBX_OK;
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (results)", who);
  if ((uintptr_t)results & 7) return hbx_fail(HBX_ERR_ARG, "%s: results must be 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  if (C == 0) {  // nothing to score: B headers with count 0
    hipLaunchKernelGGL(groups_topk_empty_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (char*)results, B,
                       k);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !bw_good || !bw_bad || !nlev_good || !nlev_bad ||
      !cand || !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const int64_t need = hbx_kde_groups_topk_workspace_bytes(B, C, k, D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  if ((uintptr_t)workspace & 15) return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
  GrpArgs A = grp_args(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad, cand, 1,
                       C, nullptr, workspace);
  GrpTopk K;
  K.out = (char*)results;
  K.pdf = (double2*)((char*)workspace + GRP_WS_HEAD + B * C * (int64_t)sizeof(GScreen));  // behind the screen slots
  K.k = k;
  K.cap = grp_topk_cap(k);
  grp_launch_screen<false>(A, s);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(groups_topk_kernel, dim3((unsigned)B), dim3(GRP_SEL_THREADS), (size_t)K.cap * 16, s, A, K);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_groups_batch_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D) {
  if (D < 1 || D > HBX_MAX_D || !grp_counts_ok(B, S, C)) return -1;
  return GRP_WS_HEAD + B * S * C * (int64_t)sizeof(GScreen);
}

int64_t hbx_kde_groups_workspace_bytes(int64_t B, int64_t C, int32_t D) {
  return hbx_kde_groups_batch_workspace_bytes(B, 1, C, D);
}

int hbx_kde_acquire_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                           const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                           const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                           const int32_t* nlev_bad, const double* cand, int64_t C, void* results, void* workspace,
                           int64_t ws_bytes, void* stream) {
  return grp_acquire("hbx_kde_acquire_groups", X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad,
                     nlev_good, nlev_bad, cand, 1, C, results, workspace, ws_bytes, stream);
}

int hbx_kde_acquire_groups_batch(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                 const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                 const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                 const int32_t* nlev_bad, const double* cand, int64_t S, int64_t C, void* results,
                                 void* workspace, int64_t ws_bytes, void* stream) {
  return grp_acquire("hbx_kde_acquire_groups_batch", X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad,
                     nlev_good, nlev_bad, cand, S, C, results, workspace, ws_bytes, stream);
}

// the grouped workspace (the screen slots) followed by the re-scored candidates' pdfs, 16 bytes per candidate: the
// ranking's entries refer to them by index, so the spill does not grow with k
int64_t hbx_kde_groups_topk_workspace_bytes(int64_t B, int64_t C, int32_t k, int32_t D) {
  if (k < 1 || k > HBX_TOPK_MAX_K) return -1;
  const int64_t base = hbx_kde_groups_batch_workspace_bytes(B, 1, C, D);
  return base < 0 ? -1 : base + B * C * (int64_t)sizeof(double2);
}

int hbx_kde_acquire_groups_topk(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                const int32_t* nlev_bad, const double* cand, int64_t C, int32_t k, void* results,
                                void* workspace, int64_t ws_bytes, void* stream) {
  return grp_acquire_topk("hbx_kde_acquire_groups_topk", X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good,
                          bw_bad, nlev_good, nlev_bad, cand, C, k, results, workspace, ws_bytes, stream);
}

}  // extern "C"
