// hbx_groups_logpdf_signed.hip -- grouped ln-pdf, the signed log-space pass (HBX_LOGPDF_SIGNED): KDEs with a negative
// Aitchison-Aitken match factor (a categorical bandwidth h > 1; status HBX_GRP_SIGNED_L / _G) summed as a signed sum
// in log space, exact only where the sum cancels.  hbx_groups_logpdf.hip has the call, the other passes and the
// contract; without the flag such a KDE goes through the exact pdf for every candidate and this file is not reached.
//
// glp_signed_kernel<DCP, DUP, NW, EXP64>: glp_f64_kernel's work split and staging.  A block is one 64-candidate tile
// of one (group, KDE), lane = candidate, its scaled coordinates (fp64) and codes (fp32) in registers; the NW waves take
// the KDE's rows in rounds of 32 per wave, each gathered through `order`, scaled and staged in the wave's LDS slice
// (DCP doubles and DUP floats per row) and read back as broadcasts, one barrier pair per round.  Per pair, fp64,
// direct differences:
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
  static_assert(DUP <= 32, "a pair's match bits are one 32-bit word");
  constexpr int NT = 64 * NW, OB = 32;   // observations per wave and round
  constexpr int RB = DCP * 8 + DUP * 4;  // bytes per staged row: DCP scaled coordinates (f64), DUP codes (f32)
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
  if (wave == 0) {
    int dc, du;
    grp_slots(A.M, lane, s_cdim, s_udim, &dc, &du);  // (dc <= DCP, du <= DUP: the status kernel checked the bucket)
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
  // per-slot constants: a_c = 1 / (h sqrt 2); delta_u (header), ln(h / (c - 1)) summed into the constant
  for (int k = tid; k < DCP; k += NT) s_sa[k] = k < dc ? 1.0 / (bw[s_cdim[k]] * 1.4142135623730951) : 0.0;
  for (int u = tid; u < DUP; u += NT) {
    double v = 0.0;
    if (u < du) {
      const int d = s_udim[u];
      const double a = 1.0 - bw[d];
      v = a == 0.0 ? -INFINITY : log(fabs(a)) - log(bw[d] / (double)(nlev[d] - 1));
    }
    s_dl[u] = v;
  }
  __syncthreads();
  if (tid == 0) {  // in slot order (deterministic)
    double lc = -log((double)nk), sad = 0.0;
    uint32_t neg = 0u;
    for (int k = 0; k < dc; ++k) lc -= log(bw[s_cdim[k]]) + 0.91893853320467274178;  // ln(h sqrt(2 pi))
    for (int u = 0; u < du; ++u) {
      const int d = s_udim[u];
      lc += log(bw[d] / (double)(nlev[d] - 1));
      if (1.0 - bw[d] < 0.0) neg |= 1u << u;
      if (s_dl[u] > -INFINITY) sad += fabs(s_dl[u]);
    }
    s_lconst = lc;
    s_sad = sad;
    s_neg = neg;
  }
  __syncthreads();
  const uint32_t neg = __builtin_amdgcn_readfirstlane(s_neg);
  const int dcq = (dc + 3) >> 2, duq = (du + 3) >> 2;
  const double* x = A.cand + (b * A.C + (valid ? i : (int64_t)tile * 64)) * D;
  double xc[DCP];
  float xu[DUP];
#pragma unroll
  for (int k = 0; k < DCP; ++k) xc[k] = k < dc ? x[s_cdim[k]] * s_sa[k] : 0.0;
#pragma unroll
  for (int u = 0; u < DUP; ++u) xu[u] = u < du ? cand_code(x[s_udim[u]]) : 0.f;
  char* wrow = srow + (size_t)wave * OB * RB;
  for (int e = lane; e < OB * RB / 4; e += 64) ((float*)wrow)[e] = 0.f;  // (the padding slots stay 0: delta 0, mask 0)
  double m = -INFINITY, Sp = 0.0, Sn = 0.0;
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
      uint32_t mb = 0u;  // the pair's match bits, slot u at bit u
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
          const bool e0 = xu[4 * q] == v.x, e1 = xu[4 * q + 1] == v.y, e2 = xu[4 * q + 2] == v.z,
                     e3 = xu[4 * q + 3] == v.w;
          t += e0 ? s_dl[4 * q] : 0.0;
          t += e1 ? s_dl[4 * q + 1] : 0.0;
          t += e2 ? s_dl[4 * q + 2] : 0.0;
          t += e3 ? s_dl[4 * q + 3] : 0.0;
          mb |= (e0 ? 1u : 0u) << (4 * q) | (e1 ? 2u : 0u) << (4 * q) | (e2 ? 4u : 0u) << (4 * q) |
                (e3 ? 8u : 0u) << (4 * q);
        }
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
