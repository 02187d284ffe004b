// hbx_topk.hip -- top-k acquisition on MI355X (gfx950): the k best candidates of ONE pool, ranked exactly.
//
// hbx_kde_acquire answers "which candidate minimises s = max(1e-8, g) / max(l, 1e-8)" (bohb.py:149-152);
// hbx_kde_acquire_topk (at the end of this file) returns the first min(k, F) entries of the stable ascending order of s
// over the F candidates whose score is not NaN: ordered by (s[i], i), every value the reference's fp64 bit
// for bit.  The scoring launch, its rescue pass and split merge, and the exact fp64 re-score are the
// argmin's, unchanged; this file holds the three steps that differ:
//
//   topk_bounds      one thread per candidate: its score interval [lo, hi] (ln units, score_interval -- the
//                    combine kernel's arithmetic), lo as the shortlist predicate reads it, hi as an ordered
//                    32-bit key.  NaN scores: lo = NaN, hi = +inf.  Candidates whose factors are both
//                    clamped (score exactly 1) get lo = hi = 0 and are ordinary members: the argmin's
//                    "only the first exact tie can win" shortcut (first1) does not hold for k > 1.
//   topk_hist (x4)   radix select of U_k, the k-th smallest finite hi, over the keys' four 8-bit digits from
//                    the top: per-block LDS histogram of the keys matching the digits already chosen, one
//                    atomic add per non-empty bin per block; each pass re-derives the earlier digits from
//                    their histograms (a 256-bin scan per block: no launch between the passes)
//   topk_shortlist   the last digit, then {i : lo[i] is not NaN and (overflow flag or lo[i] <= U_k)} -> list,
//                    one atomic add per wave.  Fewer than k finite hi: U_k = +inf, every rankable candidate.
//   (kde_exact_kernel / kde_exact_combine_kernel, hbx_exact.hip: the fp64 pdfs of the listed candidates)
//   topk_final       one block: scores from the exact pdfs, a running best-(k+1) by (score bits, index) over
//                    a shortlist of any length (bitonic merges in LDS, a threshold skipping what cannot
//                    enter), the ranked records, and HBX_ACQ_NEAR_TIE
//
// Why the shortlist holds the whole top-k.  Every candidate's true score lies in its [lo, hi] (the bounds are
// rigorous: they are what makes the argmin exact).  At least k candidates have hi <= U_k, so at least k true
// scores are <= U_k, so the k-th smallest true score is <= U_k.  Every member of the true top-k -- ties by
// index included, because a tied candidate has the same true score -- therefore has a true score <= U_k, hence
// lo <= U_k, and is re-scored.  The final ranking is over exact scores only, so candidates the shortlist
// holds beyond the top-k cost time, never correctness.  With the overflow flag (a pdf bound past fp64's exp
// range) or fewer than k finite upper bounds, every candidate with a non-NaN lo is re-scored.
//
// Result block (hbx_kde_topk_result_bytes(k) = 16 + 40 k bytes, include/hbx.h):
//   header {i32 count, i32 shortlist, i32 flags, i32 k}, then `count` records of 40 bytes
//   {i64 index, f64 score, f64 pdf_l, f64 pdf_g, f32 rel, i32 0}
#include "hbx_acq_impl.h"
#include "hbx_acquire.h"
#include "hbx_topk_rank.h"

#define TOPK_KEY_INF 0xFF800000u  // hbx_f2ord(+inf): keys below it are finite upper bounds
#define TOPK_HIST_WORDS (4 * 256)  // workspace of the k-th bound's radix select: 4 histograms of 256 bins

__global__ __launch_bounds__(256) void topk_bounds_kernel(const KdeEst* __restrict__ el,
                                                          const KdeEst* __restrict__ eg, int64_t Nc,
                                                          float* __restrict__ lo, uint32_t* __restrict__ hik,
                                                          int32_t* __restrict__ flags, uint32_t* __restrict__ hist) {
  if (blockIdx.x == 0)  // the select's histograms (its passes are later launches)
    for (int j = threadIdx.x; j < TOPK_HIST_WORDS; j += 256) hist[j] = 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool of = false;
  if (i < Nc) {
    const ScoreIv v = score_interval(el[i], eg[i]);
    of = v.of;
    // inf - inf in a bound (both pdf bounds overflowed; the flag is set then): nothing known
    const float l = v.lnan ? NAN : (v.slo == v.slo ? v.slo : -INFINITY);
    const float h = (v.lnan || v.shi != v.shi) ? INFINITY : v.shi;
    lo[i] = l;
    hik[i] = hbx_f2ord(h);
  }
  if (__ballot(of) != 0 && (threadIdx.x & 63) == 0) atomicOr(flags, HBX_ACQ_OVERFLOW);  // rare
}

// The select's state after `npass` passes, from their histograms (whole block of 256 threads): the chosen
// digits as the key's top bits, and the rank still to find among the keys that match them; rank 0xffffffff:
// fewer than k finite keys (then no digit is chosen).
struct TopkSel {
  uint32_t prefix, rank;
};
__device__ TopkSel topk_resolve(const uint32_t* __restrict__ hist, int32_t k, int npass) {
  __shared__ uint32_t sc[256];
  __shared__ TopkSel st;
  const int t = threadIdx.x;
  if (t == 0) st = TopkSel{0u, (uint32_t)k};
  __syncthreads();
  for (int q = 0; q < npass; ++q) {
    const uint32_t c = hist[q * 256 + t];
    sc[t] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan over the 256 bins
      const uint32_t v = t >= off ? sc[t - off] : 0u;
      __syncthreads();
      sc[t] += v;
      __syncthreads();
    }
    const uint32_t incl = sc[t], excl = incl - c, rank = st.rank;
    __syncthreads();
    if (rank != 0xffffffffu) {
      if (excl < rank && rank <= incl) st = TopkSel{st.prefix | ((uint32_t)t << (24 - 8 * q)), rank - excl};
      if (t == 255 && incl < rank) st.rank = 0xffffffffu;  // (first pass only: its total counts every finite key)
    }
    __syncthreads();
  }
  return st;
}

#define TOPK_HIST_PER_BLOCK 4096  // keys per block of a select pass
__global__ __launch_bounds__(256) void topk_hist_kernel(const uint32_t* __restrict__ hik, int64_t Nc, int32_t k,
                                                        int pass, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  const TopkSel sel = topk_resolve(hist, k, pass);  // (its barriers order the zeroing before the adds)
  if (sel.rank == 0xffffffffu) return;              // uniform
  const int shift = 24 - 8 * pass;
  const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
  const int64_t b0 = (int64_t)blockIdx.x * TOPK_HIST_PER_BLOCK;
#pragma unroll 4
  for (int r = 0; r < TOPK_HIST_PER_BLOCK / 256; ++r) {
    const int64_t i = b0 + r * 256 + threadIdx.x;
    if (i < Nc) {
      const uint32_t key = hik[i];
      if (key < TOPK_KEY_INF && ((key ^ sel.prefix) & himask) == 0) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(hist + pass * 256 + threadIdx.x, c);
}

#define TOPK_SHORT_PER_BLOCK 1024
__global__ __launch_bounds__(256) void topk_shortlist_kernel(const float* __restrict__ lo, int64_t Nc, int32_t k,
                                                             const uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ U,
                                                             const int32_t* __restrict__ flags,
                                                             int32_t* __restrict__ list, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ rescue_cnt) {
  const TopkSel sel = topk_resolve(hist, k, 4);
  const uint32_t uk = sel.rank == 0xffffffffu ? TOPK_KEY_INF : sel.prefix;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *U = uk;
    if (rescue_cnt) *rescue_cnt = 0;  // as kde_shortlist_kernel: the marker count starts the next call at 0
  }
  const float u = hbx_ord2f(uk);
  const bool all = (flags[0] & 1) != 0;
  const int lane = threadIdx.x & 63;
  const int64_t b0 = (int64_t)blockIdx.x * TOPK_SHORT_PER_BLOCK;
  for (int r = 0; r < TOPK_SHORT_PER_BLOCK / 256; ++r) {
    const int64_t i = b0 + r * 256 + threadIdx.x;
    bool in = false;
    if (i < Nc) {
      const float l = lo[i];
      in = l == l && (all || l <= u);
    }
    const uint64_t b = __ballot(in);
    if (b == 0) continue;  // whole wave
    int base = 0;
    if (lane == 0) base = atomicAdd(count, (int)__popcll(b));  // one add per wave
    base = __shfl(base, 0);
    if (in) list[base + __popcll(b & ((1ull << lane) - 1))] = (int32_t)i;
  }
}

// ------------------------------------------------------------------------------------------
// the final ranking

#define TOPK_T 512        // threads of the final block
#define TOPK_CAP 2048     // entries of its LDS array: <= k + 1 kept + pending ones
static_assert(HBX_TOPK_MAX_K + 1 + TOPK_T <= TOPK_CAP, "a chunk fits behind the kept entries after a merge");

__global__ __launch_bounds__(TOPK_T) void topk_final_kernel(
    const int32_t* __restrict__ list, const int32_t* __restrict__ count, const double* __restrict__ exact_l,
    const double* __restrict__ exact_g, const int32_t* __restrict__ flags, int64_t index_base, int32_t k,
    const KdeParams* __restrict__ Pg, const KdeParams* __restrict__ Pb, const KdeEst* __restrict__ el,
    const KdeEst* __restrict__ eg, TopkHead* __restrict__ head, TopkRec* __restrict__ rec) {
  // the running best-(k+1) (hbx_topk_rank.h): entries (score bits, candidate index, shortlist position)
  __shared__ uint64_t sk[TOPK_CAP];
  __shared__ int32_t si[TOPK_CAP];
  __shared__ int32_t sp[TOPK_CAP];
  __shared__ int32_t swc[TOPK_T / 64];
  const int t = threadIdx.x;
  const int cnt = *count;
  TopkRank<TOPK_T> rank;
  rank.init(sk, si, sp, swc, TOPK_CAP, k + 1);  // the k best and the best excluded one (the near-tie test's last pair)
  for (int base = 0; base < cnt; base += TOPK_T) {
    const int p = base + t;
    bool acc = false;
    uint64_t key = 0;
    int32_t idx = 0;
    if (p < cnt) {
      const double s = bohb_score(exact_g[p], exact_l[p]);
      if (s == s) {  // NaN scores are never returned
        key = (uint64_t)__double_as_longlong(s);
        idx = list[p];
        acc = rank.enters(key, idx);
      }
    }
    rank.push(acc, key, idx, p);
  }
  rank.finish();
  const int nb = rank.nb;
  const int nout = nb < k ? nb : k;
  // the ranked records; HBX_ACQ_NEAR_TIE: an entry and the next one (the last returned one's next is the
  // best excluded entry, position k) cannot be told apart by the re-score's error bounds
  bool near = false;
  for (int j = t; j < nout; j += TOPK_T) {
    const int32_t idx = si[j], p = sp[j];
    const double s = __longlong_as_double((long long)sk[j]);
    const double r = score_rel(Pg, Pb, el, eg, idx);
    TopkRec o;
    o.index = (int64_t)idx + index_base;
    o.score = s;
    o.pdf_l = exact_l[p];
    o.pdf_g = exact_g[p];
    o.rel = (float)r;
    o.pad = 0;
    rec[j] = o;
    if (j + 1 < nb) {
      const double s2 = __longlong_as_double((long long)sk[j + 1]);
      near = near || near_best(s2, score_rel(Pg, Pb, el, eg, si[j + 1]), s, r);
    }
  }
  const int any_near = __syncthreads_or(near);
  if (t == 0) {
    TopkHead hd;
    hd.count = nout;
    hd.shortlist = cnt;
    hd.flags = *flags | (any_near ? HBX_ACQ_NEAR_TIE : 0);
    hd.k = k;
    *head = hd;
  }
}

// ------------------------------------------------------------------------------------------
// launchers and entry points

// score intervals from the (merged, rescued) estimates: lo[i] as the shortlist predicate reads it, the
// ordered key of hi into hik[i]; the overflow rule into flags[0]; zeroes the select's histograms
static int hbx_topk_bounds(const KdeEst* el, const KdeEst* eg, int64_t Nc, float* lo, uint32_t* hik, int32_t* flags,
                    uint32_t* hist, hipStream_t s) {
  hipLaunchKernelGGL(topk_bounds_kernel, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, el, eg, Nc, lo, hik,
                     flags, hist);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// U[0] = the k-th smallest finite hi (+inf with fewer than k), then the shortlist {i: lo[i] == lo[i] &&
// (flags[0] & 1 || lo[i] <= U[0])} into list / count; zeroes the scoring launch's marker count
static int hbx_topk_shortlist(const float* lo, const uint32_t* hik, int64_t Nc, int32_t k, uint32_t* hist, uint32_t* U,
                       const int32_t* flags, int32_t* list, int32_t* count, int32_t* rescue_cnt, hipStream_t s) {
  if (hik) {  // the radix select (no keys: an exact-only acquisition, its histograms zero, U_k = +inf)
    const unsigned gh = (unsigned)((Nc + TOPK_HIST_PER_BLOCK - 1) / TOPK_HIST_PER_BLOCK);
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(topk_hist_kernel, dim3(gh), dim3(256), 0, s, hik, Nc, k, pass, hist);
      HBX_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(topk_shortlist_kernel, dim3((unsigned)((Nc + TOPK_SHORT_PER_BLOCK - 1) / TOPK_SHORT_PER_BLOCK)),
                     dim3(256), 0, s, lo, Nc, k, (const uint32_t*)hist, U, flags, list, count, rescue_cnt);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// the k smallest (score, index) of the re-scored shortlist, ranked, into the result block
static int hbx_topk_final(const int32_t* list, const int32_t* count, const double* exact_l, const double* exact_g,
                   const int32_t* flags, int64_t index_base, int32_t k, const KdeParams* Pg, const KdeParams* Pb,
                   const KdeEst* el, const KdeEst* eg, void* results, hipStream_t s) {
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "top-k: k=%d outside [1, %d]", k, HBX_TOPK_MAX_K);
  hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(TOPK_T), 0, s, list, count, exact_l, exact_g, flags,
                     index_base, k, Pg, Pb, el, eg, (TopkHead*)results, (TopkRec*)((char*)results + sizeof(TopkHead)));
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

// The workspace is hbx_kde_acquire's (the near list's 4 Nc bytes hold the upper bounds' keys) followed by the
// radix select's histograms.
int64_t hbx_kde_topk_workspace_bytes(int64_t Nc, int32_t k, int64_t nmax) {
  if (Nc < 0 || k < 1 || k > HBX_TOPK_MAX_K) return -1;
  return (int64_t)(ws_layout(Nc, nmax).total + 4 * TOPK_HIST_WORDS);
}

int64_t hbx_kde_topk_result_bytes(int32_t k) {
  if (k < 1 || k > HBX_TOPK_MAX_K) return -1;
  return 16 + 40 * (int64_t)k;
}

// The k best candidates of one pool by (score, index): the scoring launch, its rescue pass and split merge and
// the exact re-score as the argmin runs them for one acquisition (acq_score, acq_exact: hbx_acquire.h); between
// them the bounds pass, the k-th smallest upper bound and the shortlist against it, after them the ranking.
// Unlike the argmin, the combine never does the rescue, the exact re-score never scans and its unit sums are
// always combined by their own launch.
int hbx_kde_acquire_topk(const double* cand, int64_t Nc, int32_t k, int64_t index_base, const void* pair,
                         void* results, void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_acquire_topk";
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const KdePairRef* pp = acq_pair(who, pair);
  if (!pp) return HBX_ERR_ARG;
  const KdePairRef& p = *pp;
  int rc = acq_check(who, p, cand, Nc, workspace);
  if (rc) return rc;
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, HBX_TOPK_MAX_K);
  if (p.D < 1 || p.D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d", who, p.D);
  const int64_t need = hbx_kde_topk_workspace_bytes(Nc, k, p.nmax);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "workspace too small: %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  if (Nc == 0) {  // count = 0 and no launch: a zeroed header
    HBX_HIP(hipMemsetAsync(results, 0, 16, s));
    return HBX_OK;
  }
  AcqPlan plan;
  rc = acq_plan(p, true, &plan);
  if (rc) return rc;
  const WsLayout w = ws_layout(Nc, p.nmax);
  const AcqWs a(workspace, w);
  uint32_t* hik = (uint32_t*)a.near;                         // the upper bounds' keys in the near list's place
  uint32_t* hist = (uint32_t*)((char*)workspace + w.total);  // the select's histograms after the argmin's workspace
  // (no timing events; the rescue pass always a launch of its own: the bounds pass does not rescue)
  const ScoreRequest rq{cand, Nc, p.D, nullptr, a.rescue, a.init(), p.nmax, false, s};
  ScoreResult sr;
  rc = acq_score(plan, p, a, rq, 0, &sr);
  if (rc) return rc;
  if (plan.exact_only) {  // no estimates: every candidate re-scored (lo = 0, the flag set), no select
    rc = acq_exact_only_init(Nc, (uint32_t)Nc, a, s);
    if (rc) return rc;
    HBX_HIP(hipMemsetAsync(hist, 0, 4 * TOPK_HIST_WORDS, s));
  } else {
    rc = hbx_topk_bounds(a.el, a.eg, Nc, a.lo, hik, a.flags, hist, s);
    if (rc) return rc;
  }
  rc = hbx_topk_shortlist(a.lo, plan.exact_only ? nullptr : hik, Nc, k, hist, a.U, a.flags, a.list, a.count, a.rescue,
                          s);
  if (rc) return rc;
  rc = acq_exact(p, cand, Nc, a, false, true, s);
  if (rc) return rc;
  return hbx_topk_final(a.list, a.count, a.exact_l, a.exact_g, a.flags, index_base, k, p.Pg(), p.Pb(), a.el, a.eg,
                        results, s);
}

}  // extern "C"
