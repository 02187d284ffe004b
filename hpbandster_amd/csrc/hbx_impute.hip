// hbx_impute.hip -- conditional search spaces on the device: the imputed view of B groups' good / bad sets, and
// the deactivation of proposed rows.  The rules are in hbx_impute.h, shared with the host entries below.
//
// hbx_kde_impute_groups.  One workgroup per (group, set), one launch:
//   A   items (word w, dim d), d fastest: the 32 rows of word w are read through the split order (coalesced across
//       d), copied to the view as they are, and their non-NaN bits at d become mask[w][d]; the d == 0 item also
//       writes order_v / src_v of its rows
//   A2  one thread per dim: the per-word prefix counts and m_d
//   B   one thread per row that holds a NaN: imp_row, which overwrites the NaN entries of its view row
// The masks live in LDS where (2 W + 1) D words fit IMP_LDS_WORDS (config #5: W = 27, D = 32 -> 7 KB), else in the
// workgroup's own slots of the workspace; HBX_IMPUTE_LDS=0 sends every set to the workspace (tests).  Only
// __syncthreads between the phases: a workgroup reads nothing another one wrote.  counts is zeroed by a
// stream-ordered memset ahead of the launch and takes one atomic add per workgroup.
//
// Workspace: slots of 2 D words (mask, prefix), set (b, s) starting at slot (first view row >> 5) + 2 b + s -- W
// slots per set never reach the next set's first slot --, T = (Nv >> 5) + 2 B + 2 slots in all, then m_d of every
// set, u32[2 B][D].
#include <string.h>

#include <vector>

#include "hbx_impute.h"

#define IMP_THREADS 256
#define IMP_LDS_WORDS 8192  // 32 KB

static inline int64_t imp_slots(int64_t Nv, int64_t B) { return (Nv >> 5) + 2 * B + 2; }

// What a (group, set) is.  0: nothing to write; < 0: the view does not match the sizes; 1: impute.
struct ImpPlan {
  int64_t ns, vbase, v0, ord_off, row0;
};
__host__ __device__ inline int imp_plan(const int64_t* seg_off, const int64_t* n_good, const int64_t* n_bad,
                                        const int64_t* view_off, int64_t Nv, int64_t b, int set, ImpPlan* P) {
  const int64_t s0 = seg_off[b], n = seg_off[b + 1] - s0, ng = n_good[b], nb = n_bad[b];
  const int64_t v0 = view_off[b], v1 = view_off[b + 1];
  const bool model = ng > 0 && ng <= n && nb > 0 && nb <= n;  // hbx_kde_fit's skip rule
  const int64_t want = model ? ng + nb : 0;
  if (v0 < 0 || v1 > Nv || v1 - v0 != want || n > INT32_MAX) return -1;
  if (!model) return 0;
  P->ns = set ? nb : ng;
  P->v0 = v0;
  P->vbase = v0 + (set ? ng : 0);
  P->ord_off = s0 + (set ? n - nb : 0);
  P->row0 = s0;
  return 1;
}

__global__ __launch_bounds__(IMP_THREADS) void impute_groups_kernel(
    const double* __restrict__ X, int32_t D, const int64_t* __restrict__ seg_off, const int64_t* __restrict__ order,
    const int64_t* __restrict__ n_good, const int64_t* __restrict__ n_bad, const int32_t* __restrict__ levels,
    const int64_t* __restrict__ view_off, int64_t Nv, uint64_t seed, uint64_t counter_base, uint32_t stream_id,
    double* Xv, int64_t* __restrict__ order_v, int32_t* __restrict__ src_v, int32_t* counts, uint32_t* ws,
    int64_t slots, int use_lds) {
  __shared__ uint32_t lds[IMP_LDS_WORDS];
  __shared__ int32_t s_any, s_donor, s_prior;
  const int64_t b = blockIdx.x >> 1;
  const int set = blockIdx.x & 1;
  const int tid = threadIdx.x;
  ImpPlan P;
  const int kind = imp_plan(seg_off, n_good, n_bad, view_off, Nv, b, set, &P);  // (uniform)
  if (kind <= 0) {
    if (kind < 0 && set == 0 && counts && tid == 0) counts[2 * b] = counts[2 * b + 1] = -1;
    return;
  }
  const int64_t ns = P.ns;
  const int W = (int)((ns + 31) >> 5);
  const int64_t WD = (int64_t)W * D;
  uint32_t *mask, *pre, *cnt;
  if (use_lds && 2 * WD + D <= IMP_LDS_WORDS) {
    mask = lds;
    pre = lds + WD;
    cnt = lds + 2 * WD;
  } else {
    mask = ws + ((P.vbase >> 5) + 2 * b + set) * 2 * (int64_t)D;
    pre = mask + WD;
    cnt = ws + slots * 2 * (int64_t)D + (2 * b + set) * (int64_t)D;
  }
  const double* Xs = X + P.row0 * (int64_t)D;
  const int64_t* ord = order + P.ord_off;
  double* out = Xv + P.vbase * (int64_t)D;
  if (tid == 0) s_any = s_donor = s_prior = 0;
  // A: copy, masks
  for (int64_t i = tid; i < WD; i += IMP_THREADS) {
    const int w = (int)(i / D), d = (int)(i - (int64_t)w * D);
    const int64_t j0 = (int64_t)w * 32;
    const int cntj = (int)(ns - j0 < 32 ? ns - j0 : 32);
    uint32_t bits = 0;
    for (int jb = 0; jb < cntj; jb += 8) {  // 8 rows at a time: the positions, then the entries, then the stores
      int64_t row[8];
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) row[u] = ord[jb + u < cntj ? j0 + jb + u : j0];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = Xs[row[u] * D + d];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int jj = jb + u;
        if (jj < cntj) {
          out[(j0 + jj) * D + d] = v[u];
          bits |= (uint32_t)(v[u] == v[u]) << jj;
          if (d == 0) {
            order_v[P.vbase + j0 + jj] = P.vbase - P.v0 + j0 + jj;
            src_v[P.vbase + j0 + jj] = (int32_t)row[u];
          }
        }
      }
    }
    mask[i] = bits;
  }
  __syncthreads();
  // A2: prefix counts
  for (int d = tid; d < D; d += IMP_THREADS) {
    uint32_t run = 0;
    for (int w = 0; w < W; ++w) {
      pre[(int64_t)w * D + d] = run;
      run += (uint32_t)__builtin_popcount(mask[(int64_t)w * D + d]);
    }
    cnt[d] = run;
    if ((int64_t)run != ns) s_any = 1;  // (every writer stores the same value)
  }
  __syncthreads();
  if (!s_any) return;  // (uniform) no NaN in the set: the view rows are the byte copies
  // B: the rows
  ImpSet S;
  S.Xs = Xs, S.ord = ord, S.ns = ns, S.D = D, S.W = W, S.mask = mask, S.pre = pre, S.cnt = cnt, S.levels = levels;
  int32_t nd = 0, np = 0;
  for (int64_t j = tid; j < ns; j += IMP_THREADS)
    imp_row(S, j, out + j * D, seed, counter_base + (uint64_t)(P.vbase + j), stream_id, &nd, &np);
  if (nd) atomicAdd(&s_donor, nd);
  if (np) atomicAdd(&s_prior, np);
  __syncthreads();
  if (tid == 0 && counts) {
    if (s_donor) atomicAdd(&counts[2 * b], s_donor);
    if (s_prior) atomicAdd(&counts[2 * b + 1], s_prior);
  }
}

__global__ __launch_bounds__(256) void rows_deactivate_kernel(double* rows, int64_t N, int32_t D,
                                                              const int32_t* __restrict__ child,
                                                              const int32_t* __restrict__ parent,
                                                              const uint64_t* __restrict__ allowed, int64_t n_cond) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < N) imp_deactivate_row(rows + r * D, D, child, parent, allowed, n_cond);
}

// the argument checks the device and the host entry share; 1: nothing to do
static int imp_check(const char* who, const void* X, int32_t D, const void* seg_off, int64_t B, const void* order,
                     const void* n_good, const void* n_bad, const void* levels, const void* view_off, int64_t Nv,
                     const void* Xv, const void* order_v, const void* src_v, const void* counts) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || Nv < 0 || B > (1ll << 30))
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld Nv=%lld", who, (long long)B, (long long)Nv);
  if (B == 0 || Nv == 0) return 1;
  if (!X || !seg_off || !order || !n_good || !n_bad || !levels || !view_off || !Xv || !order_v || !src_v)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if (((uintptr_t)X & 7) || ((uintptr_t)seg_off & 7) || ((uintptr_t)order & 7) || ((uintptr_t)n_good & 7) ||
      ((uintptr_t)n_bad & 7) || ((uintptr_t)view_off & 7) || ((uintptr_t)Xv & 7) || ((uintptr_t)order_v & 7) ||
      ((uintptr_t)levels & 3) || ((uintptr_t)src_v & 3) || ((uintptr_t)counts & 3))
    return hbx_fail(HBX_ERR_ARG, "%s: f64 / i64 pointers must be 8-byte, i32 pointers 4-byte aligned", who);
  return HBX_OK;
}

static int deact_check(const char* who, const void* rows, int64_t N, int32_t D, const void* child, const void* parent,
                       const void* allowed, int64_t n_cond) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (N < 0 || n_cond < 0 || N > (1ll << 38))
    return hbx_fail(HBX_ERR_ARG, "%s: N=%lld n_cond=%lld", who, (long long)N, (long long)n_cond);
  if (N == 0 || n_cond == 0) return 1;
  if (!rows || !child || !parent || !allowed) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if (((uintptr_t)rows & 7) || ((uintptr_t)allowed & 7) || ((uintptr_t)child & 3) || ((uintptr_t)parent & 3))
    return hbx_fail(HBX_ERR_ARG, "%s: rows and allowed must be 8-byte, child and parent 4-byte aligned", who);
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_impute_groups_workspace_bytes(int64_t Nv, int64_t B, int32_t D) {
  if (Nv < 0 || B < 0 || B > (1ll << 30) || D < 1 || D > HBX_MAX_D) return -1;
  return (imp_slots(Nv, B) * 2 + 2 * B) * (int64_t)D * 4;
}

int hbx_kde_impute_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const int64_t* n_bad, const int32_t* levels, const int64_t* view_off,
                          int64_t Nv, uint64_t seed, uint64_t counter_base, uint32_t stream_id, double* Xv,
                          int64_t* order_v, int32_t* src_v, int32_t* counts, void* workspace, int64_t ws_bytes,
                          void* stream) {
  const char* who = "hbx_kde_impute_groups";
  const int rc = imp_check(who, X, D, seg_off, B, order, n_good, n_bad, levels, view_off, Nv, Xv, order_v, src_v,
                           counts);
  if (rc) return rc < 0 ? rc : HBX_OK;
  const int64_t need = hbx_kde_impute_groups_workspace_bytes(Nv, B, D);
  if (!workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (workspace)", who);
  if ((uintptr_t)workspace & 15) return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes,
                    (long long)need);
  hipStream_t s = (hipStream_t)stream;
  if (counts) HBX_HIP(hipMemsetAsync(counts, 0, (size_t)B * 8, s));
  hipLaunchKernelGGL(impute_groups_kernel, dim3((unsigned)(2 * B)), dim3(IMP_THREADS), 0, s, X, D, seg_off, order,
                     n_good, n_bad, levels, view_off, Nv, seed, counter_base, stream_id, Xv, order_v, src_v, counts,
                     (uint32_t*)workspace, imp_slots(Nv, B), hbx_switch_on("HBX_IMPUTE_LDS") ? 1 : 0);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// the same rule in plain loops over host memory; the masks of one set at a time in host vectors
int hbx_kde_impute_groups_host(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                               const int64_t* n_good, const int64_t* n_bad, const int32_t* levels,
                               const int64_t* view_off, int64_t Nv, uint64_t seed, uint64_t counter_base,
                               uint32_t stream_id, double* Xv, int64_t* order_v, int32_t* src_v, int32_t* counts) {
  const char* who = "hbx_kde_impute_groups_host";
  const int rc = imp_check(who, X, D, seg_off, B, order, n_good, n_bad, levels, view_off, Nv, Xv, order_v, src_v,
                           counts);
  if (rc) return rc < 0 ? rc : HBX_OK;
  std::vector<uint32_t> mask, pre, cnt((size_t)D);
  for (int64_t b = 0; b < B; ++b) {
    if (counts) counts[2 * b] = counts[2 * b + 1] = 0;
    for (int set = 0; set < 2; ++set) {
      ImpPlan P;
      const int kind = imp_plan(seg_off, n_good, n_bad, view_off, Nv, b, set, &P);
      if (kind < 0 && counts) counts[2 * b] = counts[2 * b + 1] = -1;
      if (kind <= 0) break;
      const int64_t ns = P.ns;
      const int W = (int)((ns + 31) >> 5);
      mask.assign((size_t)W * D, 0u);
      pre.assign((size_t)W * D, 0u);
      const double* Xs = X + P.row0 * (int64_t)D;
      const int64_t* ord = order + P.ord_off;
      double* out = Xv + P.vbase * (int64_t)D;
      for (int64_t j = 0; j < ns; ++j) {
        const int64_t row = ord[j];
        order_v[P.vbase + j] = P.vbase - P.v0 + j;
        src_v[P.vbase + j] = (int32_t)row;
        memcpy(out + j * D, Xs + row * D, (size_t)D * 8);
        for (int d = 0; d < D; ++d) {
          const double v = Xs[row * D + d];
          if (v == v) mask[(size_t)(j >> 5) * D + d] |= 1u << (j & 31);
        }
      }
      for (int d = 0; d < D; ++d) {
        uint32_t run = 0;
        for (int w = 0; w < W; ++w) {
          pre[(size_t)w * D + d] = run;
          run += (uint32_t)__builtin_popcount(mask[(size_t)w * D + d]);
        }
        cnt[d] = run;
      }
      ImpSet S;
      S.Xs = Xs, S.ord = ord, S.ns = ns, S.D = D, S.W = W, S.mask = mask.data(), S.pre = pre.data();
      S.cnt = cnt.data(), S.levels = levels;
      int32_t nd = 0, np = 0;
      for (int64_t j = 0; j < ns; ++j)
        imp_row(S, j, out + j * D, seed, counter_base + (uint64_t)(P.vbase + j), stream_id, &nd, &np);
      if (counts) counts[2 * b] += nd, counts[2 * b + 1] += np;
    }
  }
  return HBX_OK;
}

int hbx_rows_deactivate(double* rows, int64_t N, int32_t D, const int32_t* child, const int32_t* parent,
                        const uint64_t* allowed, int64_t n_cond, void* stream) {
  const int rc = deact_check("hbx_rows_deactivate", rows, N, D, child, parent, allowed, n_cond);
  if (rc) return rc < 0 ? rc : HBX_OK;
  hipLaunchKernelGGL(rows_deactivate_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows,
                     N, D, child, parent, allowed, n_cond);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

int hbx_rows_deactivate_host(double* rows, int64_t N, int32_t D, const int32_t* child, const int32_t* parent,
                             const uint64_t* allowed, int64_t n_cond) {
  const int rc = deact_check("hbx_rows_deactivate_host", rows, N, D, child, parent, allowed, n_cond);
  if (rc) return rc < 0 ? rc : HBX_OK;
  for (int64_t r = 0; r < N; ++r) imp_deactivate_row(rows + r * D, D, child, parent, allowed, n_cond);
  return HBX_OK;
}

}  // extern "C"
