// hbx_rescue_impl.h -- the rescue of one candidate, device code.  Users: hbx_score.hip (the rescue kernels
// behind every scoring launch) and hbx_kde.hip (kde_combine_kernel<_, true> rescues its own marked
// candidates).  The body is a header-level __device__ template so each kernel stays defined in one unit; the
// acquisition picks its combine instance from the variant's sign bit itself (ScoreFns holds no combine kernel).
#pragma once
#include "hbx_kde_impl.h"

// Rescue (rare): candidates whose every term sits far below the static bound M0 are recomputed
// with a true maximum (two passes over the observations), one candidate per thread on the VALU.
// Continuous coordinates come from the table's f32 part, categorical codes straight from the data.
// LOWREG (the combine kernel's copy): the same operations in the same order over k < dc only (the padded
// k >= dc terms add exact zeros), candidate and observation coordinates recomputed per pair instead of held
// in DCP-long register arrays -- the combine kernel keeps its occupancy (29-32 VGPRs, not up to 170)
template <int DCP, bool SIGNED, bool LOWREG = false>
__device__ __forceinline__ KdeEst kde_rescue_one(const double* __restrict__ cand, int64_t i, int32_t D,
                                                 const KdeParams* __restrict__ P) {
  constexpr int NC = DCP > 0 && !LOWREG ? DCP : 1;
  const double* x = cand + i * (int64_t)D;
  const int n = P->n, dc = P->dc, du = P->du;
  const double* __restrict__ Xo = P->X;
  const int64_t* __restrict__ rows = P->rows;
  float xs[NC], ci = 0.f, bnd = 0.f;
  auto coord = [&](const double* r, int k) { return (float)(P->cont_scale[k] * (r[P->cont_dim[k]] - P->center[k])); };
  if constexpr (LOWREG) {
#pragma unroll 1
    for (int k = 0; k < dc; ++k) {
      const float v = coord(x, k);
      ci = fmaf(-v, v, ci);
      bnd = fmaf(fabsf(2.f * v), P->xmax[k], bnd);
    }
  }
#pragma unroll
  for (int k = 0; k < (LOWREG ? 0 : DCP); ++k) {
    float v = 0.f;
    if (k < dc) v = (float)(P->cont_scale[k] * (x[P->cont_dim[k]] - P->center[k]));
    ci = fmaf(-v, v, ci);
    xs[k] = 2.f * v;
    if (k < dc) bnd = fmaf(fabsf(xs[k]), P->xmax[k], bnd);
  }
  auto pair_t = [&](int j, float& par) -> float {
    // observation row rebuilt exactly as kde_table_kernel writes it (f32 X', f64 C_j rounded once)
    const double* xo = Xo + rows[j] * (int64_t)D;
    float Xp[NC];
    double Cd = 0.0;
    if constexpr (LOWREG) {
#pragma unroll 1
      for (int k = 0; k < dc; ++k) {
        const float v = coord(xo, k);
        Cd -= (double)v * (double)v;
      }
    }
#pragma unroll
    for (int k = 0; k < (LOWREG ? 0 : DCP); ++k) {
      float v = 0.f;
      if (k < dc) v = (float)(P->cont_scale[k] * (xo[P->cont_dim[k]] - P->center[k]));
      Cd -= (double)v * (double)v;
      Xp[k] = v;
    }
    const float Cj = (float)(Cd + P->lb_sum - P->m0_log2);
    float t = fmaf(1.f, Cj, 0.f);
    t = fmaf(ci, 1.f, t);
    if constexpr (LOWREG) {
#pragma unroll 1
      for (int k = 0; k < dc; ++k) t = fmaf(2.f * coord(x, k), coord(xo, k), t);
    }
#pragma unroll
    for (int k = 0; k < (LOWREG ? 0 : DCP); ++k) t = fmaf(xs[k], Xp[k], t);
    par = 0.f;
    for (int u = 0; u < du; ++u) {
      const int d = P->cat_dim[u];
      const float m = (x[d] == xo[d]) ? 1.f : 0.f;
      t = fmaf(P->cat_delta[u], m, t);
      if (SIGNED) par = fmaf(m, P->cat_negf[u], -fabsf(par));
    }
    return t;
  };
  float mx = -INFINITY, par;
  for (int j = 0; j < n; ++j) mx = fmaxf(mx, pair_t(j, par));
  float S = 0.f, Sn = 0.f;
  if (mx > -INFINITY) {
    for (int j0 = 0; j0 < n; j0 += OBS_CHUNK) {
      float Sb = 0.f, Snb = 0.f;
      for (int j = j0; j < min(n, j0 + OBS_CHUNK); ++j) {
        const float e = __builtin_amdgcn_exp2f(pair_t(j, par) - mx);
        Sb += e;
        if (SIGNED) Snb = fmaf(fabsf(par), e, Snb);
      }
      S += Sb;
      Sn += Snb;
    }
  } else {
    mx = 0.f;
  }
  return finish_est(P, S, Sn, mx, false, ci, bnd, SIGNED, OBS_CHUNK);
}
