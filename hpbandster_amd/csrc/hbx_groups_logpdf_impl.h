// hbx_groups_logpdf_impl.h -- what the grouped ln-pdf's two files share (hbx_groups_logpdf.hip: the status kernel, the
// fp32, fp64 and exact passes and the entry point; hbx_groups_logpdf_signed.hip: the signed log-space pass): the
// launch arguments, the workspace header and the status bits of one KDE; the KDE's row view and the slot sort; and what
// glp_f64_kernel and glp_signed_kernel have in common ("the fp64 tile passes" below), compiled into each file under
// that file's own flags.
#pragma once
#include "hbx_groups_impl.h"

#define GLP_HEAD 256  // workspace header: the four counters (u64) in its first 32 bytes
#define GLP_BAD (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED)
#define GLP_EXACT_BIT(kd) ((kd) ? HBX_GRP_EXACT_G : HBX_GRP_EXACT_L)     // every value through the exact pdf
#define GLP_SIGNED_BIT(kd) ((kd) ? HBX_GRP_SIGNED_G : HBX_GRP_SIGNED_L)  // the signed pass, its list through the exact pdf

struct GlpArgs {
  GrpModel M;
  const double* cand;
  int64_t C;
  int32_t tiles;     // ceil(C / 64)
  int32_t kd0;       // first KDE of the launch's grid.y (0: good / ln_l, 1: bad / ln_g)
  int32_t fp64_only;
  int32_t signed_route;  // HBX_LOGPDF_SIGNED: KDEs with a negative match factor take the signed pass
  double rtol;
  double* out[2];    // ln_l, ln_g (nullable)
  int32_t* status;
  unsigned long long* stat;  // the header's counters
  int32_t* cnt;              // [B][2] listed candidates per (group, KDE)
  int32_t* list;             // [B][2][C]
};

// The lanes of one wave that hold a candidate without a written value (`listed`) append their indices i to the
// (group, KDE)'s list segment: one atomic per tile; the segment holds C entries and a candidate is listed once.
__device__ __forceinline__ void glp_list_append(const GlpArgs& A, int64_t b, int kd, bool listed, int64_t i, int lane) {
  const uint64_t bal = __ballot(listed);
  if (!bal) return;
  const int first = __ffsll((long long)bal) - 1;
  int32_t base = 0;
  if (lane == first) base = atomicAdd(&A.cnt[b * 2 + kd], __popcll(bal));
  base = __shfl(base, first);
  if (listed) A.list[(b * 2 + kd) * A.C + base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)i;
}

// KDE kd of group b: its row count, the group's observations, the KDE's row positions in them, bandwidths, levels
struct GlpKde {
  int64_t nk;
  const double* Xs;
  const int64_t* rows;
  const double* bw;
  const int32_t* nlev;
};

__device__ __forceinline__ GlpKde glp_kde(const GrpModel& M, int64_t b, int kd) {
  const int64_t s0 = M.seg_off[b], n = M.seg_off[b + 1] - s0;
  GlpKde V;
  V.nk = kd ? M.n_bad[b] : M.n_good[b];
  V.Xs = M.X + s0 * M.D;
  V.rows = M.order + s0 + (kd ? n - V.nk : 0);
  V.bw = (kd ? M.bw_bad : M.bw_good) + b * M.D;
  V.nlev = (kd ? M.nlev_bad : M.nlev_good) + b * M.D;
  return V;
}

// The dims sorted into slots by wave 0 (dc <= DCP, du <= DUP: the status kernel checked the bucket), the counts
// through s_i[0 .. 2) to every wave; whole block, ends with a barrier.
__device__ __forceinline__ void glp_slots(const GrpModel& M, int32_t* s_cdim, int32_t* s_udim, int32_t* s_i, int* dc,
                                          int* du) {
  if (threadIdx.x < 64) {
    grp_slots(M, threadIdx.x, s_cdim, s_udim, dc, du);
    if (threadIdx.x == 0) {
      s_i[0] = *dc;
      s_i[1] = *du;
    }
  }
  __syncthreads();
  *dc = s_i[0];
  *du = s_i[1];
}

// ---- the fp64 tile passes (glp_f64_kernel, glp_signed_kernel) ------------------------------------------------
// What the two passes share: a block is one 64-candidate tile of one (group, KDE), lane = candidate, its scaled
// coordinates (fp64) and codes (fp32) in registers; the NW waves take the KDE's rows in rounds of GLP_OB per wave, each
// gathered through `order`, scaled and staged in the wave's LDS slice (DCP doubles, then DUP floats per row) and read
// back as broadcasts, one barrier pair per round.  Each pass keeps its own accumulator, merge, bound and epilogue.
#define GLP_OB 32                                // observations per wave and round
#define GLP_RB(DCP, DUP) ((DCP) * 8 + (DUP) * 4)  // bytes per staged row

// Per-slot constants of KDE V (whole block, NT threads, ends with a barrier): s_sa = a_c = 1 / (h sqrt 2); s_dl =
// delta_u = ln|1 - h| - ln(h / (c - 1)), what a match adds to ln(h / (c - 1)), itself summed into *s_lconst with the
// normaliser (kde_logpdf_tiled_kernel's constant).  One formula for both passes: for h < 1 it is ln(1 - h) - ..., the
// same double; h == 1 gives -inf either way (a matching term is exactly 0); h > 1 reaches the signed pass alone.
// SIGNED: also *s_sad = sum_u |delta_u| over the finite deltas and *s_neg = the mask of the slots with h > 1.
template <int DCP, int DUP, int NT, bool SIGNED>
__device__ __forceinline__ void glp_slot_consts(const GlpKde& V, int dc, int du, const int32_t* s_cdim,
                                                const int32_t* s_udim, double* s_sa, double* s_dl, double* s_lconst,
                                                double* s_sad, uint32_t* s_neg) {
  const int tid = threadIdx.x;
  for (int k = tid; k < DCP; k += NT) s_sa[k] = k < dc ? 1.0 / (V.bw[s_cdim[k]] * 1.4142135623730951) : 0.0;
  for (int u = tid; u < DUP; u += NT) {
    double v = 0.0;
    if (u < du) {
      const int d = s_udim[u];
      const double a = 1.0 - V.bw[d];
      v = a == 0.0 ? -INFINITY : log(fabs(a)) - log(V.bw[d] / (double)(V.nlev[d] - 1));
    }
    s_dl[u] = v;
  }
  if constexpr (SIGNED) __syncthreads();  // (thread 0 reads s_dl)
  if (tid == 0) {  // in slot order (deterministic)
    double lc = -log((double)V.nk), sad = 0.0;
    uint32_t neg = 0u;
    for (int k = 0; k < dc; ++k) lc -= log(V.bw[s_cdim[k]]) + 0.91893853320467274178;  // ln(h sqrt(2 pi))
    for (int u = 0; u < du; ++u) {
      const int d = s_udim[u];
      lc += log(V.bw[d] / (double)(V.nlev[d] - 1));
      if constexpr (SIGNED) {
        if (1.0 - V.bw[d] < 0.0) neg |= 1u << u;
        if (s_dl[u] > -INFINITY) sad += fabs(s_dl[u]);
      }
    }
    *s_lconst = lc;
    if constexpr (SIGNED) {
      *s_sad = sad;
      *s_neg = neg;
    }
  }
  __syncthreads();
}

// A lane's candidate x in registers, and the wave's LDS slice zeroed (the padding slots stay 0: delta 0, no match bit)
template <int DCP, int DUP>
__device__ __forceinline__ void glp_load_cand64(const double* x, int dc, int du, const int32_t* s_cdim,
                                                const int32_t* s_udim, const double* s_sa, char* wrow, int lane,
                                                double (&xc)[DCP], float (&xu)[DUP]) {
#pragma unroll
  for (int k = 0; k < DCP; ++k) xc[k] = k < dc ? x[s_cdim[k]] * s_sa[k] : 0.0;
#pragma unroll
  for (int u = 0; u < DUP; ++u) xu[u] = u < du ? cand_code(x[s_udim[u]]) : 0.f;
  for (int e = lane; e < GLP_OB * GLP_RB(DCP, DUP) / 4; e += 64) ((float*)wrow)[e] = 0.f;
}

// One wave stages rows [j0, j0 + jmax) of KDE V into its slice; a row's slots by consecutive lanes.  The callers put
// a block-wide barrier before (the previous round is read) and after it.
template <int DCP, int DUP>
__device__ __forceinline__ void glp_stage64(const GlpKde& V, int D, int dc, const int32_t* s_cdim, const int32_t* s_udim,
                                            const double* s_sa, int64_t j0, int jmax, char* wrow, int lane) {
  constexpr int RB = GLP_RB(DCP, DUP);
  for (int e = lane; e < jmax * D; e += 64) {
    const int r = e / D, k = e - r * D;
    const double* xr = V.Xs + V.rows[j0 + r] * (int64_t)D;
    if (k < dc)
      ((double*)(wrow + r * RB))[k] = xr[s_cdim[k]] * s_sa[k];
    else
      ((float*)(wrow + r * RB + DCP * 8))[k - dc] = (float)xr[s_udim[k - dc]];  // (an integer in [0, 1024): exact)
  }
}

// The pair exponent of this lane's candidate against one staged row, ln units: an fma chain over the continuous
// slots' direct differences in four-slot pieces (dcq, duq: the live pieces, uniform), then s_dl[u] per matching code.
// BITS: *mb = the pair's match bits, slot u at bit u (DUP <= 32).
template <int DCP, int DUP, bool BITS>
__device__ __forceinline__ double glp_pair_t64(const char* row, int dcq, int duq, const double (&xc)[DCP],
                                               const float (&xu)[DUP], const double* s_dl, uint32_t* mb) {
  static_assert(!BITS || DUP <= 32, "a pair's match bits are one 32-bit word");
  const double2* rc = (const double2*)row;
  const float4* ru = (const float4*)(row + DCP * 8);
  double t = 0.0;
  [[maybe_unused]] uint32_t bits = 0u;
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
      const bool e0 = xu[4 * q] == v.x, e1 = xu[4 * q + 1] == v.y, e2 = xu[4 * q + 2] == v.z, e3 = xu[4 * q + 3] == v.w;
      t += e0 ? s_dl[4 * q] : 0.0;
      t += e1 ? s_dl[4 * q + 1] : 0.0;
      t += e2 ? s_dl[4 * q + 2] : 0.0;
      t += e3 ? s_dl[4 * q + 3] : 0.0;
      if constexpr (BITS)
        bits |= (e0 ? 1u : 0u) << (4 * q) | (e1 ? 2u : 0u) << (4 * q) | (e2 ? 4u : 0u) << (4 * q) |
                (e3 ? 8u : 0u) << (4 * q);
    }
  if constexpr (BITS) *mb = bits;
  return t;
}

// the signed pass's launch (hbx_groups_logpdf_signed.hip): the bucket's instance, fp64 exponentials for rtol < 1e-5
int glp_signed_launch(const GlpArgs& A, dim3 grid, hipStream_t s);
