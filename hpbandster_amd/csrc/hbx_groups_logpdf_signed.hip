// hbx_groups_logpdf_signed.hip -- grouped ln-pdf, the signed log-space pass (HBX_LOGPDF_SIGNED): KDEs with a negative
// Aitchison-Aitken match factor (a categorical bandwidth h > 1; status HBX_GRP_SIGNED_L / _G) summed as a signed sum
// in log space, exact only where the sum cancels.  hbx_groups_logpdf.hip has the call, the other passes and the
// contract; without the flag such a KDE goes through the exact pdf for every candidate and this file is not reached.
//
// glp_signed_kernel<DCP, DUP, NW, EXP64>: glp_f64_kernel's work split, staging and pair exponent, the shared pieces
// of hbx_groups_logpdf_impl.h ("the fp64 tile passes": glp_slot_consts<.., SIGNED = true>, glp_load_cand64,
// glp_stage64, glp_pair_t64<.., BITS = true>).  Per pair, fp64, direct differences:
//     t = sum_c -((x_c - X_jc) / (h_c sqrt 2))^2 + sum_u [x_u == X_ju] delta_u,   delta_u = ln|1 - h_u| - ln(h_u / (c_u - 1))
//   (delta_u = -inf where 1 - h_u == 0: a matching term is exactly 0, t = -inf and the pair adds nothing).  The
//   term's sign is the parity of its matches in slots with h > 1: the pair's match bits form one 32-bit word (DUP <=
//   32), ANDed with the KDE's negative-slot mask -- block-uniform, in an SGPR --, popcount & 1.  There is no branch on
//   the sign: two running sums S+ and S- against one shared reference point m, the running maximum of ceil(t log2 e)
//   over the terms of either sign, each term 2^(t log2 e - m) added to the sum the parity bit selects.  m is an
//   integer, so the rescale of both sums when it rises, and the merge of the waves' (m, S+, S-) -- in wave order,
//   through LDS: two runs give the same bytes -- are ldexp, exact.
// Matrix instructions do not fit: the contract's error argument rests on the direct-difference form in fp64 (an
// expanded |x|^2 - 2 x.X + |X|^2 cancels), and fp64 MFMA offers no difference-then-square.
//
// The bound.  One sum's relative error eps, kde_logpdf_tiled_kernel's argument (hbx_logpdf.hip) with the reference
// point an integer (the rescales are exact, so rises of the maximum add nothing), n the KDE's rows, M the final m:
//     the terms    x = t log2 e - m.  Terms with x >= -65: v_exp_f32 on the fp32-rounded x is off by at most
//                  ln 2 |x| 2^-24 + 2^-22 <= 2.93e-6 relative, eps_x = 3e-6; EXP64: x is an fp64 difference, 65 ln 2
//                  2^-53 + exp2's 2^-52, eps_x = 2^-46.  Terms with x < -65: true and computed below 2^-64 each (the
//                  exponent's own error E_t is required below 1/2), together n 2^-63 against S+ + S- >= 1/2.
//     the exponent t is an fma chain of dc + du steps over fp64 operands, each rounding at most 2^-53 of a partial sum
//                  bounded by |t| + 2 sad, sad = sum_u |delta_u| (finite deltas); for the terms that count |t log2 e| <=
//                  |M| + 65, so E_t = (dc + du + 2) 2^-53 (|M| + 65 + 2 sad log2 e) in log2 units, a factor within
//                  2^+-E_t <= 1 + 0.7 E_t per term.  (a = x / (h sqrt 2) and the rows' are fp64 products rounded once:
//                  the reference's own (x - X) / h carries the same rounding; not counted, as in glp_f64_kernel.)
//     the sums     fp64 additions and the merge: (n + NW) 2^-52.
//     => eps = eps_x + 0.7 E_t + (n + NW) 2^-52 + n 2^-62, per sum, relative to that sum.
//   Two sums: P = S+ - S-, |dP| <= eps (S+ + S-), so |dP / P| <= eps kappa with kappa = (S+ + S-) / |P|, and
//     |ln p_est - ln p| <= eps kappa / (1 - eps kappa) + 2^-48 (|ln P| + |M ln 2| + |lconst| + |ln p|)   (the fp64 epilogue)
//   A value ln P + M ln 2 + lconst is written when P > 0, every input and sum is finite, eps kappa < 1/2, E_t < 1/2
//   and the bound is within 0.99 rtol max(1, |ln p_est|).  Every other candidate -- P <= 0, kappa too large, NaN --
//   is appended to the (group, KDE)'s list segment (glp_list_append) and gets ln of the bit-exact fp64 pdf from
//   glp_exact_kernel's listed form.  Correctness never rests on this pass: it only decides which values the exact
//   path need not compute.  A certified candidate whose fp64 pdf underflows to 0 keeps its finite log-space value.
#include "hbx_groups_logpdf_impl.h"

template <int DCP, int DUP, int NW, bool EXP64>
__global__ __launch_bounds__(64 * NW) void glp_signed_kernel(GlpArgs A) {
  constexpr int NT = 64 * NW, OB = GLP_OB, RB = GLP_RB(DCP, DUP);
  __shared__ __align__(16) char srow[NW * OB * RB];
  __shared__ double s_sa[DCP], s_dl[DUP];
  __shared__ int32_t s_cdim[DCP], s_udim[DUP];
  __shared__ double s_pm[NW][64], s_pp[NW][64], s_pq[NW][64];
  __shared__ int32_t s_pn[NW][64];
  __shared__ int32_t s_i[2];
  __shared__ uint32_t s_neg;
  __shared__ double s_lconst, s_sad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = A.M.D;
  const int kd = A.kd0 + (int)blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int st = A.status[b];
  if ((st & GLP_BAD) || !(st & GLP_SIGNED_BIT(kd))) return;  // uniform
  const int64_t i = (int64_t)tile * 64 + lane;
  const bool valid = i < A.C;
  int dc, du;
  glp_slots(A.M, s_cdim, s_udim, s_i, &dc, &du);
  const GlpKde V = glp_kde(A.M, b, kd);
  const int64_t nk = V.nk;
  glp_slot_consts<DCP, DUP, NT, true>(V, dc, du, s_cdim, s_udim, s_sa, s_dl, &s_lconst, &s_sad, &s_neg);
  const uint32_t neg = __builtin_amdgcn_readfirstlane(s_neg);
  const int dcq = (dc + 3) >> 2, duq = (du + 3) >> 2;
  double xc[DCP];
  float xu[DUP];
  char* wrow = srow + (size_t)wave * OB * RB;
  glp_load_cand64<DCP, DUP>(A.cand + (b * A.C + (valid ? i : (int64_t)tile * 64)) * D, dc, du, s_cdim, s_udim, s_sa, wrow,
                            lane, xc, xu);
  double m = -INFINITY, Sp = 0.0, Sn = 0.0;
  bool nan = false;
  for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * OB) {  // uniform trip count: the barriers are block-wide
    __syncthreads();  // (the rows of the previous round are read)
    const int64_t j0 = c0 + (int64_t)wave * OB;
    const int jmax = (int)(nk - j0 < OB ? (nk - j0 > 0 ? nk - j0 : 0) : OB);
    glp_stage64<DCP, DUP>(V, D, dc, s_cdim, s_udim, s_sa, j0, jmax, wrow, lane);
    __syncthreads();
    for (int j = 0; j < jmax; ++j) {
      uint32_t mb;  // the pair's match bits, slot u at bit u
      const double t = glp_pair_t64<DCP, DUP, true>(wrow + j * RB, dcq, duq, xc, xu, s_dl, &mb);
      const double tl = t * 1.4426950408889634;  // log2 units
      const bool odd = __popc(mb & neg) & 1;
      double e = 0.0;
      if (tl > -INFINITY) {
        const double tc = ceil(tl);
        if (tc > m) {  // a new reference point (integer): exact rescale of both sums
          const int sh = (int)fmax(m - tc, -2000.0);
          Sp = ldexp(Sp, sh);
          Sn = ldexp(Sn, sh);
          m = tc;
        }
        e = EXP64 ? exp2(tl - m) : (double)__builtin_amdgcn_exp2f((float)(tl - m));
      } else if (tl != tl) {
        nan = true;
      }
      Sp += odd ? 0.0 : e;
      Sn += odd ? e : 0.0;
    }
  }
  s_pm[wave][lane] = m;
  s_pp[wave][lane] = Sp;
  s_pq[wave][lane] = Sn;
  s_pn[wave][lane] = nan;
  __syncthreads();
  if (wave != 0) return;
  // merge the waves' partials in wave order
  double M = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    M = fmax(M, s_pm[w][lane]);
    nan = nan || s_pn[w][lane];
  }
  double Pt = 0.0, Nt = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w)
    if (s_pm[w][lane] > -INFINITY) {
      const int sh = (int)fmax(s_pm[w][lane] - M, -2000.0);
      Pt += ldexp(s_pp[w][lane], sh);
      Nt += ldexp(s_pq[w][lane], sh);
    }
  // the bound (header), in fp64
  const double P = Pt - Nt, kappa = (Pt + Nt) / fabs(P);
  const double Et = (double)(dc + du + 2) * 0x1p-53 * (fabs(M) + 65.0 + 2.0 * s_sad * 1.4426950408889634);
  const double eps = (EXP64 ? 0x1p-46 : 3e-6) + 0.7 * Et + (double)(nk + NW) * 0x1p-52 + (double)nk * 0x1p-62;
  const double rel = eps * kappa;
  const double lnP = log(P), lnM = M * 0.69314718055994531;
  const double lp = lnP + lnM + s_lconst;
  const double bound = rel / (1.0 - rel) + 0x1p-48 * (fabs(lnP) + fabs(lnM) + fabs(s_lconst) + fabs(lp));
  const bool ok = valid && !nan && P > 0.0 && Pt - Pt == 0.0 && Nt - Nt == 0.0 && M - M == 0.0 && lp - lp == 0.0 &&
                  Et < 0.5 && rel < 0.5 && bound <= 0.99 * A.rtol * fmax(1.0, fabs(lp));
  if (ok) A.out[kd][b * A.C + i] = lp;
  const uint64_t okb = __ballot(ok);
  glp_list_append(A, b, kd, valid && !ok, i, lane);
  if (lane == 0 && okb) atomicAdd(&A.stat[1], (unsigned long long)__popcll(okb));
}

int glp_signed_launch(const GlpArgs& A, dim3 grid, hipStream_t s) {
#define GLP_LAUNCH_SG(DCP, DUP, NW, DT) \
  hipLaunchKernelGGL((glp_signed_kernel<DCP, DUP, NW, true>), grid, dim3(64 * NW), 0, s, A)
#define GLP_LAUNCH_SG_EXP32(DCP, DUP, NW, DT) \
  hipLaunchKernelGGL((glp_signed_kernel<DCP, DUP, NW, false>), grid, dim3(64 * NW), 0, s, A)
  if (A.rtol < 1e-5)
    GRP_BUCKET_LAUNCH(A.M.D, GLP_LAUNCH_SG);
  else
    GRP_BUCKET_LAUNCH(A.M.D, GLP_LAUNCH_SG_EXP32);
#undef GLP_LAUNCH_SG
#undef GLP_LAUNCH_SG_EXP32
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}
