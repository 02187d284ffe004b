// hbx_kde.hip -- KDE acquisition on MI355X (gfx950): l(x)/g(x) scoring of candidates against the
// good/bad product-kernel KDEs of BOHB, and the exact argmin.
//
// Reference path: bohb.py:124-152 calls statsmodels KDEMultivariate.pdf
// (SM:kernel_density.py:162-196 -> SM:_kernel_base.py:456-518 gpke -> SM:kernels.py:23-65,108-125)
// twice per candidate and keeps the first candidate with the smallest max(f,g)/max(l,f), f = the pair's score floor
// (hbx_kde_pair_set_rules; 1e-8, the reference's, unless set).
//
// Engine structure (one acquisition, all on one HIP stream, no host round trip until the result):
//   acq_init         U = +inf, counters = 0
//   kde_logpdf<..>   x2 (good, bad): fp32 log-domain sum over observations, one candidate per lane,
//                    observations broadcast through the scalar path; per candidate ln S+, ln S-, bound
//                    (hbx_score.hip dispatches, hbx_score_*.hip hold the kernels)
//                    -- or, for a large single acquisition without ln-pdf outputs, the staged scoring
//                    (hbx_staged.hip): l for every candidate, g only where l alone does not rule the
//                    candidate out; the others carry an l-only interval through the steps below
//   kde_combine      per-candidate score interval [lo, hi] (ln units) + block min of hi -> U
//   kde_shortlist    every candidate with lo <= U (the only ones that can be the argmin)
//   kde_exact        fp64 re-score of the shortlist in the reference's arithmetic/operation order (hbx_exact.hip)
//   kde_final        strict-'<', first-index argmin over the exact scores
// hbx_kde_acquire_topk (the k best of one pool) runs the same scoring and exact re-score (acq_score, acq_exact)
// around its own bounds / k-th bound / shortlist / ranking steps: hbx_topk.hip.
#include "hbx_acquire.h"

#include <string.h>

#include <new>

#include "hbx_acq_impl.h"
#include "hbx_host.h"
#include "hbx_pairwise.h"
#include "hbx_rescue_impl.h"

// ------------------------------------------------------------------------------------------
// score intervals, shortlist, exact re-score, final argmin

__global__ void acq_init_kernel(uint32_t* U, int32_t* count, int32_t* flags, int32_t* first1, AcqResult* res) {
  if (threadIdx.x == 0 && blockIdx.x == 0) acq_init_state(U, count, flags, first1, res);
}

// batched acquisition: per-segment bound, flags, shortlist count, best score and (index, position) key
__global__ void acq_init_batch_kernel(int64_t B, uint32_t* __restrict__ U, int32_t* __restrict__ flags,
                                      int32_t* __restrict__ segcnt, uint64_t* __restrict__ best,
                                      uint64_t* __restrict__ key, int32_t* __restrict__ first1,
                                      int32_t* __restrict__ count, int32_t* __restrict__ segnear) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) *count = 0;
  if (b < B) {
    U[b] = hbx_f2ord(INFINITY);
    flags[b] = 0;
    segcnt[b] = 0;
    segnear[b] = 0;
    first1[b] = INT32_MAX;
    best[b] = ~0ull;
    key[b] = ~0ull;
  }
}

// Candidates [b*seg, (b+1)*seg) form acquisition b (seg = Nc: one acquisition).  U[b] = min over the
// segment of the upper score bound, flags[b] bit 0 = overflow risk (re-score the whole segment).
// Candidates whose l and g are both certainly below the score floor f (1e-8 by default) score exactly f/f = 1
// (bohb.py:129):
// they tie, so only the first of them per segment (first1[b]) can win and needs the exact re-score
// (BOHB's own sampler puts most candidates there at D = 32: the truncnorm scale is 3 bw).
// (OBS_SPLIT_MAX, the observation splits of one scoring launch at most: hbx_score.h)

// (merge_splits, a candidate's estimate merged over its observation-split partials: hbx_acq_impl.h, shared with
// the staged acquisition's kernels)

// observation splits: each candidate's partial estimates merged into its first slot, for the combine and
// every later step (one thread per candidate and KDE; launched only when the scoring launch split)
__global__ __launch_bounds__(256) void kde_merge_splits_kernel(KdeEst* __restrict__ el, KdeEst* __restrict__ eg,
                                                               int64_t Nc, int32_t ns_l, int32_t ns_g) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * Nc) return;
  const bool g = t >= Nc;
  const int64_t i = g ? t - Nc : t;
  const int ns = g ? ns_g : ns_l;
  if (ns > 1) (g ? eg : el)[i] = merge_splits(g ? eg : el, Nc, i, ns);
}

#ifndef COMBINE_SUB
#define COMBINE_SUB 2  // 256-candidate sub-blocks per block of kde_combine_kernel (2: 13-15 us at 1e6, 4: 15-17, 8: 19)
#endif
// RESCUE: the rescue pass done here (a single acquisition scored by a 32x32 pair launch without splits):
// with the scoring launch's marker count non-zero, a thread re-scores its own marked candidates before
// combining them (kde_rescue_one, the rescue kernel's arithmetic) and stores them for the later steps --
// one launch less per acquisition (a rescue launch took 4.8 us even when it exited at once)
struct CombineRescue {
  const double* cand;
  int32_t D;
  const KdeParams* Pl;  // the KDEs behind el / eg
  const KdeParams* Pg;
  const int32_t* cnt;   // the scoring launch's marker count
};
template <bool SIGNED, bool RESCUE>
__global__ __launch_bounds__(256) void kde_combine_kernel(KdeEst* __restrict__ el, KdeEst* __restrict__ eg,
                                                          int64_t Nc, uint32_t seg, float* __restrict__ logl,
                                                          float* __restrict__ logg, float* __restrict__ lo,
                                                          uint32_t* __restrict__ U, int32_t* __restrict__ flags,
                                                          int32_t* __restrict__ first1, CombineRescue rs,
                                                          ScoreFloor F) {
  // COMBINE_SUB consecutive 256-candidate sub-blocks per block: every sub-block's loads are issued first
  // (the kernel is latency-bound with one candidate per thread), then each runs as its own block would
  // the marker count, final since the scoring launch ended: a plain (scalar) load, like the estimates'
  int32_t nres = 0;
  if constexpr (RESCUE) nres = *rs.cnt;
  KdeEst ea[COMBINE_SUB], eb[COMBINE_SUB];
#pragma unroll
  for (int r = 0; r < COMBINE_SUB; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * COMBINE_SUB + r) * 256 + threadIdx.x;
    if (i < Nc) {
      ea[r] = el[i];
      eb[r] = eg[i];
    }
  }
  if constexpr (RESCUE) {
    if (nres != 0) {  // rare
#pragma unroll
      for (int r = 0; r < COMBINE_SUB; ++r) {
        const int64_t i = ((int64_t)blockIdx.x * COMBINE_SUB + r) * 256 + threadIdx.x;
        if (i < Nc && ea[r].err == -1.f) {
          ea[r] = kde_rescue_one<0, SIGNED, true>(rs.cand, i, rs.D, rs.Pl);
          el[i] = ea[r];
        }
        if (i < Nc && eb[r].err == -1.f) {
          eb[r] = kde_rescue_one<0, SIGNED, true>(rs.cand, i, rs.D, rs.Pg);
          eg[i] = eb[r];
        }
      }
    }
  }
  __shared__ float rh[COMBINE_SUB][4];
  __shared__ int32_t rf[COMBINE_SUB][4];
  // thread 0: the whole-block sub-blocks' minima of one segment, lowered into U / first1 once per segment
  // (an atomic round trip per sub-block made thread 0 -- and the next sub-block's barrier -- wait 4x)
  uint32_t acc_sg = ~0u;
  float acc_h = INFINITY;
  int32_t acc_f = INT32_MAX;
#pragma unroll
  for (int r = 0; r < COMBINE_SUB; ++r) {
    const int64_t blkr = (int64_t)blockIdx.x * COMBINE_SUB + r;
    if (blkr * 256 >= Nc) break;  // uniform
    const int64_t i = blkr * 256 + threadIdx.x;
    float h = INFINITY;
    bool one = false;
    const uint32_t sg = (uint32_t)(i < Nc ? i : Nc - 1) / seg;
    if (i < Nc) {
      // (score_interval: hbx_acq_impl.h, shared with the top-k bounds pass)
      // (a staged acquisition's candidates without g: the interval l alone gives)
      const ScoreIv v = eb[r].err == HBX_EST_NOT_EVAL ? score_interval_l_only(ea[r], F) : score_interval(ea[r], eb[r], F);
      const float lpt = v.lpt, gpt = v.gpt;
      const bool of = v.of;
      // an exact tie at 1 is excluded from the shortlist unless it is the segment's first (first1)
      const float slo = v.one ? NAN : v.slo;
      if (!v.lnan) h = v.shi;
      one = v.one;
      if (logl) logl[i] = lpt;
      if (logg) logg[i] = gpt;
      lo[i] = slo;  // (the upper bound only enters the segment minimum below)
      if (of) atomicOr(flags + sg, 1);
    }
    // min of hi and first exact tie per segment.  Same-address atomics serialise in L2 (~10 ns each),
    // so: block reduction when the block lies in one segment (the common case), one wave-level atomic
    // when the wave does, per lane otherwise; and an atomic only when it can still lower the value.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t blk0 = blkr * 256;
    const int64_t blk1 = (blk0 + 255 < Nc ? blk0 + 255 : Nc - 1);
    auto lower_u = [&](uint32_t sgi, float hv) {
      const uint32_t o = hbx_f2ord(hv);
      if (hv < INFINITY && o < __hip_atomic_load(U + sgi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(U + sgi, o);
    };
    auto lower_first = [&](uint32_t sgi, int32_t iv) {
      if (iv < __hip_atomic_load(first1 + sgi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first1 + sgi, iv);
    };
    const uint32_t s0 = __shfl(sg, 0), s63 = __shfl(sg, 63);
    if (s0 == s63) {
      for (int o = 32; o > 0; o >>= 1) h = fminf(h, __shfl_xor(h, o));
      const uint64_t ones = __ballot(one);
      const int32_t f1 = ones ? (int32_t)(blk0 + 64 * wv + __ffsll((long long)ones) - 1) : INT32_MAX;
      if ((uint32_t)(blk0 / seg) == (uint32_t)(blk1 / seg)) {
        if (lane == 0) {
          rh[r][wv] = h;
          rf[r][wv] = f1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          const float hb = fminf(fminf(rh[r][0], rh[r][1]), fminf(rh[r][2], rh[r][3]));
          const int32_t fb = min(min(rf[r][0], rf[r][1]), min(rf[r][2], rf[r][3]));
          if (sg != acc_sg) {
            if (acc_sg != ~0u) {
              lower_u(acc_sg, acc_h);
              if (acc_f != INT32_MAX) lower_first(acc_sg, acc_f);
            }
            acc_sg = sg;
            acc_h = hb;
            acc_f = fb;
          } else {
            acc_h = fminf(acc_h, hb);
            acc_f = min(acc_f, fb);
          }
        }
      } else if (lane == 0) {
        lower_u(sg, h);
        if (f1 != INT32_MAX) lower_first(sg, f1);
      }
    } else {
      lower_u(sg, h);
      if (one) lower_first(sg, (int32_t)i);
    }
  }  // sub-block
  if (threadIdx.x == 0 && acc_sg != ~0u) {
    const uint32_t o = hbx_f2ord(acc_h);
    if (acc_h < INFINITY && o < __hip_atomic_load(U + acc_sg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(U + acc_sg, o);
    if (acc_f != INT32_MAX &&
        acc_f < __hip_atomic_load(first1 + acc_sg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(first1 + acc_sg, acc_f);
  }
}

typedef void (*combine_fn)(KdeEst*, KdeEst*, int64_t, uint32_t, float*, float*, float*, uint32_t*, int32_t*,
                           int32_t*, CombineRescue, ScoreFloor);

__global__ __launch_bounds__(256) void kde_shortlist_kernel(const float* __restrict__ lo, int64_t Nc, uint32_t seg,
                                                            const uint32_t* __restrict__ U,
                                                            const int32_t* __restrict__ flags,
                                                            int32_t* __restrict__ list,
                                                            int32_t* __restrict__ count,
                                                            int32_t* __restrict__ segcnt,
                                                            const int32_t* __restrict__ first1,
                                                            int32_t* __restrict__ rescue_cnt) {
  // the rescue of this acquisition is done (its pass or the combine): the marker count starts the next at 0
  if (rescue_cnt && blockIdx.x == 0 && threadIdx.x == 0) *rescue_cnt = 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Nc) return;
  const uint32_t sg = (uint32_t)i / seg;
  const float u = hbx_ord2f(U[sg]);
  const bool all = (flags[sg] & 1) != 0;
  const float l = lo[i];
  if ((l == l && (all || l <= u)) || (int32_t)i == first1[sg]) {
    const int pos = atomicAdd(count, 1);
    list[pos] = (int32_t)i;
    if (segcnt) atomicAdd(segcnt + sg, 1);
  }
}

// A get_config pick published to device-mapped host memory by the final argmin (hbx_kde_acquire_bound with err /
// row_out): the record, whether any of the call's candidates hit a sampler domain error, the winning row (as
// tagged 8-byte words: kde_final_kernel)
struct PickOut {
  const double* cand;
  const uint8_t* err;  // nullable
  int64_t Nc;
  int32_t D;
  char* out;  // null: no pick
};

// the final argmin of one acquisition (256 threads): the split re-score's unit sums -> pdfs, strict '<'
// first-index argmin over the shortlist, the near set, the result record
__global__ __launch_bounds__(256) void kde_final_kernel(const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ count,
                                                        const double* exact_l,  // (written here through exact_lw / _gw)
                                                        const double* exact_g, const int32_t* __restrict__ flags,
                                                        int64_t index_base, const KdeParams* __restrict__ Pg,
                                                        const KdeParams* __restrict__ Pb,
                                                        const KdeEst* __restrict__ el, const KdeEst* __restrict__ eg,
                                                        int32_t* __restrict__ near_list, AcqResult* __restrict__ res,
                                                        int32_t nbuf, const double* __restrict__ part,
                                                        double* exact_lw, double* exact_gw, AcqResult* host_res,
                                                        int32_t seq, PickOut pick, double pfloor) {
  __shared__ double bs[256];
  __shared__ AcqResult rec_sh;
  __shared__ int64_t bi[256];
  __shared__ int32_t bp[256];
  __shared__ double exl[256], exg[256];  // the exact pdfs of a shortlist of <= 256 (no global re-read)
  __shared__ double rb_sh;
  __shared__ int32_t nnear;
  const int cnt = *count;
  int err_any = 0;
  if (pick.out && pick.err) {  // uniform
    bool e = false;
    for (int64_t i = threadIdx.x; i < pick.Nc; i += 256) e = e || pick.err[i] != 0;
    err_any = __syncthreads_or(e);
  }
  // shortlists of <= 256 (the common case): thread p owns candidate p -- its index and bound are loaded
  // first, beside the unit sums' combination, and its pdfs come back through LDS
  const bool small = cnt <= 256;
  const int tp = threadIdx.x;
  const int64_t my_idx = (small && tp < cnt) ? list[tp] : 0;
  const double my_rel = (small && tp < cnt) ? score_rel(Pg, Pb, el, eg, my_idx) : 0.0;
  if (part && cnt <= EXACT_SPLIT_CAP) {  // the split re-score's unit sums -> pdfs (kde_exact_combine's work)
    for (int pk = threadIdx.x >> 6; pk < 2 * cnt; pk += 4) {  // one wave per (candidate, KDE)
      const bool isl = pk & 1;
      const int n = (isl ? Pg : Pb)->n;
      const double* us = part + (int64_t)pk * nbuf * PW_SPLIT_UNITS;
      double acc = 0.0;
      for (int c = 0, b = 0; c < n; c += PW_BUF, ++b) {
        const int m = (n - c) < PW_BUF ? (n - c) : PW_BUF;
        acc = acc + pw_combine_units_wave<PW_SPLIT_CUT>(m, us + b * PW_SPLIT_UNITS);
      }
      if ((threadIdx.x & 63) == 0) {
        const double pdf = acc / (double)n;
        (isl ? exact_lw : exact_gw)[pk >> 1] = pdf;
        if (small) (isl ? exl : exg)[pk >> 1] = pdf;
      }
    }
    __threadfence_block();
    __syncthreads();
  } else if (small) {  // pdfs written by another kernel: one global read each
    if (tp < cnt) {
      exl[tp] = exact_l[tp];
      exg[tp] = exact_g[tp];
    }
    __syncthreads();
  }
  double best = INFINITY;
  int64_t bidx = INT64_MAX;
  int32_t bpos = -1;
  if (threadIdx.x == 0) nnear = 0;
  for (int p = threadIdx.x; p < cnt; p += 256) {
    const double s = bohb_score(small ? exg[p] : exact_g[p], small ? exl[p] : exact_l[p], pfloor);
    const int64_t idx = small ? my_idx : list[p];
    // valid iff s < +inf (bohb.py:150 'val < best' with best = inf); strict '<', first index wins
    if (s < INFINITY && (s < best || (s == best && idx < bidx))) {
      best = s;
      bidx = idx;
      bpos = p;
    }
  }
  bs[threadIdx.x] = best;
  bi[threadIdx.x] = bidx;
  bp[threadIdx.x] = bpos;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      const double s2 = bs[threadIdx.x + w];
      const int64_t i2 = bi[threadIdx.x + w];
      if (s2 < bs[threadIdx.x] || (s2 == bs[threadIdx.x] && i2 < bi[threadIdx.x])) {
        bs[threadIdx.x] = s2;
        bi[threadIdx.x] = i2;
        bp[threadIdx.x] = bp[threadIdx.x + w];
      }
    }
    __syncthreads();
  }
  // the near set: every re-scored candidate the winner cannot be told apart from by these bounds
  const int32_t wp = bp[0];
  double rb = 0.0;
  if (small) {  // the winner's thread holds its bound
    if (tp == wp) rb_sh = my_rel;
    __syncthreads();
    if (wp >= 0) rb = rb_sh;
  }
  if (wp >= 0) {
    const double sb = bs[0];
    if (!small) rb = score_rel(Pg, Pb, el, eg, list[wp]);
    for (int p = threadIdx.x; p < cnt; p += 256) {
      const double s = bohb_score(small ? exg[p] : exact_g[p], small ? exl[p] : exact_l[p], pfloor);
      const int64_t ip = small ? my_idx : list[p];
      if (p == wp || near_best(s, small ? my_rel : score_rel(Pg, Pb, el, eg, ip), sb, rb))
        near_list[atomicAdd(&nnear, 1)] = (int32_t)ip;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    AcqResult r;  // acq_init_state's record when nothing is finite
    r.index = -1;
    r.score = r.pdf_l = r.pdf_g = NAN;
    r.shortlist = cnt;
    r.flags = *flags | (nnear > 1 ? HBX_ACQ_NEAR_TIE : 0);
    r.near = nnear;
    r.rel = (float)rb;
    if (wp >= 0) {
      r.index = bi[0] + index_base;
      r.score = bs[0];
      r.pdf_l = small ? exl[wp] : exact_l[wp];
      r.pdf_g = small ? exg[wp] : exact_g[wp];
    }
    *res = r;
    rec_sh = r;
  }
  if (host_res || pick.out) {  // uniform: the record (and a pick's flag and row) to mapped host memory
    static_assert(sizeof(AcqResult) % 4 == 0, "record of whole words");
    __syncthreads();
    // every 32-bit word as one 8-byte system-scope store tagged with the call's sequence number (seq << 32 |
    // word): the host takes each word only once its tag is the call's, so there is no acknowledgement wait
    // and no completion word (wait_tagged)
    uint64_t* out = (uint64_t*)(pick.out ? pick.out : (char*)host_res);
    const uint64_t tag = (uint64_t)(uint32_t)seq << 32;
    constexpr int RW = (int)(sizeof(AcqResult) / 4);
    if (threadIdx.x < RW) hbx_publish_store64(out + threadIdx.x, tag | ((const uint32_t*)&rec_sh)[threadIdx.x]);
    if (pick.out) {  // a pick: + the domain-error flag (word RW) and the winning row (words RW + 1 ..)
      if (threadIdx.x == 0) hbx_publish_store64(out + RW, tag | (err_any ? 1u : 0u));
      const int64_t idx = rec_sh.index - index_base;
      if (rec_sh.index >= 0 && idx < pick.Nc)
        for (int w = threadIdx.x; w < 2 * pick.D; w += 256)
          hbx_publish_store64(out + RW + 1 + w, tag | ((const uint32_t*)(pick.cand + idx * pick.D))[w]);
    }
  }
}

// Batched argmin, three passes over the shortlist: (1) per-segment minimum of the exact score,
// (2) among the entries reaching it the smallest index (strict '<', first index -- bohb.py:149-152),
// (3) one thread per segment writes its record.  Scores are > 0 or NaN (both factors are clamped
// to >= the score floor; 0 where l is +inf), so the bits of a finite score order like the score.
// (bohb_score: hbx_acq_impl.h)

__global__ __launch_bounds__(256) void kde_batch_min_kernel(const int32_t* __restrict__ list,
                                                            const int32_t* __restrict__ count, uint32_t seg,
                                                            const double* __restrict__ exact_l,
                                                            const double* __restrict__ exact_g,
                                                            uint64_t* __restrict__ best, double pfloor) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *count) return;
  const double s = bohb_score(exact_g[p], exact_l[p], pfloor);
  if (s < INFINITY) atomicMin((unsigned long long*)best + (uint32_t)list[p] / seg,
                              (unsigned long long)__double_as_longlong(s));
}

__global__ __launch_bounds__(256) void kde_batch_key_kernel(const int32_t* __restrict__ list,
                                                            const int32_t* __restrict__ count, uint32_t seg,
                                                            const double* __restrict__ exact_l,
                                                            const double* __restrict__ exact_g,
                                                            const uint64_t* __restrict__ best,
                                                            uint64_t* __restrict__ key, double pfloor) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *count) return;
  const double s = bohb_score(exact_g[p], exact_l[p], pfloor);
  const uint32_t i = (uint32_t)list[p], sg = i / seg;
  if (s < INFINITY && (uint64_t)__double_as_longlong(s) == best[sg])
    atomicMin((unsigned long long*)key + sg, ((unsigned long long)(i - sg * seg) << 32) | (uint32_t)p);
}

// per shortlist entry: 1 in near_flag (and counted in segnear) when its segment's winner cannot be
// told apart from it by the error bounds (kde_final_kernel's near set, per segment)
__global__ __launch_bounds__(256) void kde_batch_near_kernel(const int32_t* __restrict__ list,
                                                             const int32_t* __restrict__ count, uint32_t seg,
                                                             const double* __restrict__ exact_l,
                                                             const double* __restrict__ exact_g,
                                                             const uint64_t* __restrict__ key,
                                                             const KdeParams* __restrict__ Pg,
                                                             const KdeParams* __restrict__ Pb,
                                                             const KdeEst* __restrict__ el,
                                                             const KdeEst* __restrict__ eg,
                                                             int32_t* __restrict__ near_flag,
                                                             int32_t* __restrict__ segnear, double pfloor) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *count) return;
  const uint32_t i = (uint32_t)list[p], sg = i / seg;
  const uint64_t k = key[sg];
  int f = 0;
  if (k != ~0ull) {
    const int wp = (int)(uint32_t)k;
    const double sb = bohb_score(exact_g[wp], exact_l[wp], pfloor);
    const double rb = score_rel(Pg, Pb, el, eg, list[wp]);
    const double s = bohb_score(exact_g[p], exact_l[p], pfloor);
    f = (p == wp || near_best(s, score_rel(Pg, Pb, el, eg, i), sb, rb)) ? 1 : 0;
  }
  near_flag[p] = f;
  if (f) atomicAdd(segnear + sg, 1);
}

__global__ __launch_bounds__(256) void kde_batch_final_kernel(int64_t B, const uint64_t* __restrict__ key,
                                                              const int32_t* __restrict__ segcnt,
                                                              const int32_t* __restrict__ flags,
                                                              const int32_t* __restrict__ segnear,
                                                              const int32_t* __restrict__ list,
                                                              const double* __restrict__ exact_l,
                                                              const double* __restrict__ exact_g,
                                                              const KdeParams* __restrict__ Pg,
                                                              const KdeParams* __restrict__ Pb,
                                                              const KdeEst* __restrict__ el,
                                                              const KdeEst* __restrict__ eg,
                                                              int64_t index_base, AcqResult* __restrict__ res,
                                                              double pfloor) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  AcqResult r;
  r.shortlist = segcnt[b];
  r.near = segnear[b];
  r.flags = flags[b] | (r.near > 1 ? HBX_ACQ_NEAR_TIE : 0);
  r.rel = 0.f;
  const uint64_t k = key[b];
  if (k == ~0ull) {
    r.index = -1;
    r.score = NAN;
    r.pdf_l = NAN;
    r.pdf_g = NAN;
  } else {
    const int p = (int)(uint32_t)k;
    r.index = (int64_t)(k >> 32) + index_base;
    r.pdf_l = exact_l[p];
    r.pdf_g = exact_g[p];
    r.score = bohb_score(r.pdf_g, r.pdf_l, pfloor);
    r.rel = (float)score_rel(Pg, Pb, el, eg, list[p]);
  }
  res[b] = r;
}

// Exact-only acquisition (KDEs outside every fp32 scoring bucket): every candidate joins the fp64
// re-score -- no estimate (err = -2 marks it), each segment flagged so the shortlist takes it whole.
__global__ __launch_bounds__(256) void kde_exact_only_init_kernel(int64_t Nc, uint32_t seg, KdeEst* __restrict__ el,
                                                                  KdeEst* __restrict__ eg, float* __restrict__ lo,
                                                                  int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Nc) return;
  const KdeEst e = {0.f, -INFINITY, -2.f, 0.f};
  el[i] = e;
  eg[i] = e;
  lo[i] = 0.f;
  if ((uint32_t)i % seg == 0) flags[(uint32_t)i / seg] = HBX_ACQ_OVERFLOW;
}

// ln of the exact pdfs for the logl/logg outputs of an exact-only acquisition
__global__ __launch_bounds__(256) void kde_exact_logs_kernel(const int32_t* __restrict__ list,
                                                             const int32_t* __restrict__ count,
                                                             const double* __restrict__ exact_l,
                                                             const double* __restrict__ exact_g,
                                                             float* __restrict__ logl, float* __restrict__ logg) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *count) return;
  const int i = list[p];
  if (logl) logl[i] = (float)log(exact_l[p]);
  if (logg) logg[i] = (float)log(exact_g[p]);
}

// ------------------------------------------------------------------------------------------
// launch side

WsLayout ws_layout(int64_t Nc, int64_t nmax, int64_t B) {
  WsLayout w;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t r = o;
    o += (bytes + 255) & ~(size_t)255;
    return r;
  };
  w.res = take(sizeof(AcqResult));
  w.count = take(4);
  w.U = take(4 * B);
  w.flags = take(4 * B);
  w.segcnt = take(4 * B);
  w.segnear = take(4 * B);
  w.best = take(8 * B);
  w.key = take(8 * B);
  w.first1 = take(4 * B);
  w.rescue = take(4);
  // estimates: one per candidate and observation split (the launch's splits never exceed this bound).  The
  // allowance is non-decreasing in Nc -- a workspace sized for a larger candidate count serves every smaller
  // one: splits happen only up to 65536 candidates (128 tiles), where Nc x sp <= min(16 Nc, 196608)
  const int sp = obs_splits((unsigned)((Nc + 511) / 512), nmax, true);
  const int64_t cap16 = 16 * Nc < 196608 ? 16 * Nc : 196608;
  const int64_t nest = Nc * sp > cap16 ? Nc * sp : cap16;
  w.est_l = take(sizeof(KdeEst) * nest);
  w.est_g = take(sizeof(KdeEst) * nest);
  w.lo = take(4 * Nc);
  w.list = take(4 * Nc);
  w.near = take(4 * Nc);
  w.exact_l = take(8 * Nc);
  w.exact_g = take(8 * Nc);
  w.part = take(8 * (size_t)2 * EXACT_SPLIT_CAP * PW_SPLIT_UNITS * ((nmax + PW_BUF - 1) / PW_BUF));
  // the staged acquisition (hbx_staged.hip): lists of whole 512-candidate tiles, 4 bytes per candidate for the
  // survivor list, and the list launches' split partials
  static_assert(sizeof(AcqResult) + 4 * HBX_ST_WORDS <= 256, "the state words fit the result slot's padding");
  w.stage = w.res + sizeof(AcqResult);
  const int64_t tiles = (Nc + 511) / 512;
  w.list_cap = (int32_t)(512 * (tiles < 1 ? 1 : tiles > STAGED_LIST_CAP / 512 ? STAGED_LIST_CAP / 512 : tiles));
  w.seeds = take(4 * (size_t)w.list_cap);
  w.surv = take(4 * Nc);
  w.lpart = take(sizeof(KdeEst) * (size_t)OBS_SPLIT_MAX * w.list_cap);
  // stage 1's block maxima (staged_score_l): an area of its own, 4 bytes per 256 candidates, rather than an alias
  // of the split partials -- no block count at which the fold would have to be off, nothing to reason about when
  // another launch starts to use that area
  w.bmax = take(4 * (size_t)((Nc + 255) / 256));
  w.total = o;
  return w;
}

int acq_check(const char* who, const KdePairRef& p, const double* cand, int64_t Nc, const void* workspace) {
  if ((!cand && Nc > 0) || !p.params_good || !p.table_good || !p.X_good || !p.rows_good || !p.params_bad ||
      !p.table_bad || !p.X_bad || !p.rows_bad || !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if (Nc < 0 || Nc > INT32_MAX) return hbx_fail(HBX_ERR_ARG, "Nc=%lld out of range", (long long)Nc);
  return HBX_OK;
}

const KdePairRef* acq_pair(const char* who, const void* pair) {
  if (!pair) hbx_fail(HBX_ERR_ARG, "%s: null pair", who);
  return (const KdePairRef*)pair;
}

int acq_plan(const KdePairRef& p, bool fast, AcqPlan* plan) {
  plan->exact_only = KdeVariant::decode(p.variant_good).exact_only || KdeVariant::decode(p.variant_bad).exact_only;
  plan->fg = pick_logpdf(p.dc_pad, p.du_pad, p.variant_good, fast);
  plan->fb = pick_logpdf(p.dc_pad, p.du_pad, p.variant_bad, fast);
  if (!plan->exact_only && (!plan->fg.main || !plan->fb.main))
    return hbx_fail(HBX_ERR_UNSUPPORTED, "no kernel for dc_pad=%d du_pad=%d", p.dc_pad, p.du_pad);
  return HBX_OK;
}

int acq_score(const AcqPlan& plan, const KdePairRef& p, const AcqWs& a, const ScoreRequest& rq, int64_t batch_B,
              ScoreResult* out) {
  *out = ScoreResult{};
  const hipStream_t s = rq.s;
  const bool scored = rq.Nc > 0 && !plan.exact_only;
  if (scored) {
    const int rc = launch_score2({plan.fg, p.params_good, p.table_good, a.el},
                                 {plan.fb, p.params_bad, p.table_bad, a.eg}, rq, out);
    if (rc) return rc;
  }
  if (batch_B) {
    hipLaunchKernelGGL(acq_init_batch_kernel, dim3((unsigned)((batch_B + 255) / 256)), dim3(256), 0, s, batch_B, a.U,
                       a.flags, a.segcnt, a.best, a.key, a.first1, a.count, a.segnear);
    HBX_LAUNCH_CHECK();
  } else if (!out->inited) {  // (a single acquisition's pair launch or its rescue pass initialises the state)
    hipLaunchKernelGGL(acq_init_kernel, dim3(1), dim3(64), 0, s, a.U, a.count, a.flags, a.first1, a.res);
    HBX_LAUNCH_CHECK();
  }
  if (scored && (out->nsplit[0] > 1 || out->nsplit[1] > 1)) {  // merged before the combine / bounds pass
    hipLaunchKernelGGL(kde_merge_splits_kernel, dim3((unsigned)((2 * rq.Nc + 255) / 256)), dim3(256), 0, s, a.el,
                       a.eg, rq.Nc, out->nsplit[0], out->nsplit[1]);
    HBX_LAUNCH_CHECK();
  }
  return HBX_OK;
}

int acq_exact_only_init(int64_t Nc, uint32_t seg, const AcqWs& a, hipStream_t s) {
  hipLaunchKernelGGL(kde_exact_only_init_kernel, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, Nc, seg, a.el,
                     a.eg, a.lo, a.flags);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// One call of acquire_impl, as its entry point fills it
struct AcqCall {
  const char* who;
  const double* cand;
  int64_t Nc, seg, index_base;
  float *logl_out, *logg_out;  // nullable: the ln-pdf estimates
  AcqResult* batch_res;        // nullable: one acquisition, the record stays in the workspace
  void* workspace;
  int64_t ws_bytes;
  void *events, *stream;
  // the bound call's publish target in mapped host memory: the record alone (host_res) or a pick (pick.out),
  // tagged with the call's sequence number; neither: nothing published
  AcqResult* host_res;
  int32_t seq;
  PickOut pick;
};

// Shared body of hbx_kde_acquire (batch_res == nullptr: one acquisition over all Nc candidates, the
// record stays in the workspace) and hbx_kde_acquire_batch (B = ceil(Nc/seg) acquisitions over
// consecutive segments of seg candidates, one record each into batch_res).
static int acquire_impl(const void* pair, const AcqCall& c) {
  const KdePairRef* pp = acq_pair(c.who, pair);
  if (!pp) return HBX_ERR_ARG;
  const KdePairRef& p = *pp;
  const double* cand = c.cand;
  const int64_t Nc = c.Nc, seg = c.seg;
  float *logl_out = c.logl_out, *logg_out = c.logg_out;
  AcqResult* batch_res = c.batch_res;
  int rc = acq_check(c.who, p, cand, Nc, c.workspace);
  if (rc) return rc;
  if (seg < 1) return hbx_fail(HBX_ERR_ARG, "%s: segment length %lld", c.who, (long long)seg);
  const int64_t B = batch_res ? (Nc + seg - 1) / seg : 1;
  const WsLayout w = ws_layout(Nc, p.nmax, B);
  if ((size_t)c.ws_bytes < w.total)
    return hbx_fail(HBX_ERR_ARG, "workspace too small: %lld < %lld bytes", (long long)c.ws_bytes,
                    (long long)w.total);
  // no ln-pdf estimates returned: the fast scoring instances (their looser bounds only widen the shortlist
  // the exact re-score resolves)
  const bool fast = !logl_out && !logg_out;
  AcqPlan plan;
  rc = acq_plan(p, fast, &plan);
  if (rc) return rc;
  const AcqWs a(c.workspace, w);
  hipStream_t s = (hipStream_t)c.stream;
  hipEvent_t* ev = (hipEvent_t*)c.events;  // optional: [before l, between, after g] for timing
  const uint32_t sg = (uint32_t)(batch_res ? seg : (Nc > 0 ? Nc : 1));
  if (B == 0) return HBX_OK;  // batched call without candidates: no records
  bool rescue_inline = false;  // the rescue pass left to the combine kernel
  // Staged scoring (hbx_staged.hip): a single acquisition without ln-pdf outputs, both KDEs on the coarse 32x32
  // instance, and enough pairs that the bad KDE's walk outweighs the stages' eight extra launches (nmax stands
  // for the bad KDE's observation count, which the host does not hold).  HBX_STAGED_MIN_PAIRS: measured,
  // profiles/staged/README.md.
  const int stg = (!batch_res && fast && Nc > 0) ? hbx_staged_mode() : 0;
  const bool staged = stg && acq_staged_supported(plan) &&
                      (stg == 2 || (double)Nc * (double)p.nmax >= HBX_STAGED_MIN_PAIRS);
  // the short tail (HBX_STAGED_TAIL): the staged launches leave the intervals and the shortlist as well
  const bool tail = staged && hbx_staged_tail();
  if (staged) {
    rc = acq_score_staged(plan, p, cand, Nc, a, ev, s, tail);
    rescue_inline = true;  // marked g estimates of the list launches: the combine kernel re-scores them
  } else {
    // splits for the pick only (reported ln-pdfs stay unsplit); a batched call's rescue pass is always a launch
    const ScoreRequest rq{cand, Nc, p.D, ev, a.rescue, batch_res ? KdePairArgs::AcqInitPtrs{} : a.init(),
                          fast ? p.nmax : 0, !batch_res, s};
    ScoreResult sr;
    rc = acq_score(plan, p, a, rq, batch_res ? B : 0, &sr);
    rescue_inline = sr.rescue_inline;
  }
  if (rc) return rc;
  const dim3 grid((unsigned)((Nc + 255) / 256));
  bool fuse_combine = false;
  if (Nc > 0) {
    if (plan.exact_only) {
      rc = acq_exact_only_init(Nc, sg, a, s);
      if (rc) return rc;
    } else if (!tail) {
      const CombineRescue rs{cand, p.D, p.Pg(), p.Pb(), a.rescue};
      // the rescue pass left to the combine kernel: its instance by the sign bit (a pair launch: one for both KDEs)
      const bool sgn = KdeVariant::decode(p.variant_good).has_neg;
      const combine_fn cf = !rescue_inline ? kde_combine_kernel<false, false>
                            : sgn          ? kde_combine_kernel<true, true>
                                           : kde_combine_kernel<false, true>;
      hipLaunchKernelGGL(cf, dim3((unsigned)((Nc + 256 * COMBINE_SUB - 1) / (256 * COMBINE_SUB))), dim3(256), 0, s,
                         a.el, a.eg, Nc, sg, logl_out, logg_out, a.lo, a.U, a.flags, a.first1, rs, p.floor);
      HBX_LAUNCH_CHECK();
    }
    // a single acquisition of few candidates: the exact re-score's blocks shortlist for themselves
    // (the short tail of a staged acquisition has built the shortlist already)
    const bool scan = !batch_res && Nc <= EXACT_SCAN_MAX && !tail;
    if (!scan && !tail) {
      hipLaunchKernelGGL(kde_shortlist_kernel, grid, dim3(256), 0, s, a.lo, Nc, sg, a.U, a.flags, a.list, a.count,
                         batch_res ? a.segcnt : (int32_t*)nullptr, a.first1, a.rescue);
      HBX_LAUNCH_CHECK();
    }
    // single acquisition: the final kernel combines the unit sums itself (one launch less)
    fuse_combine = !batch_res && !(plan.exact_only && (logl_out || logg_out));
    // (behind the short tail the re-score's wide blocks: measured at the bench's shortlist of two or three; a staged
    // call with a long shortlist -- HBX_STAGED=2 on small pools, ties -- gets them too, and that case is not measured)
    rc = acq_exact(p, cand, Nc, a, scan, !fuse_combine, s, tail);
    if (rc) return rc;
    if (plan.exact_only && (logl_out || logg_out)) {
      hipLaunchKernelGGL(kde_exact_logs_kernel, grid, dim3(256), 0, s, a.list, a.count, a.exact_l, a.exact_g, logl_out,
                         logg_out);
      HBX_LAUNCH_CHECK();
    }
  }
  if (!batch_res) {
    hipLaunchKernelGGL(kde_final_kernel, dim3(1), dim3(256), 0, s, a.list, a.count, a.exact_l, a.exact_g, a.flags,
                       c.index_base, p.Pg(), p.Pb(), a.el, a.eg, a.near, a.res,
                       (int32_t)((p.nmax + PW_BUF - 1) / PW_BUF), fuse_combine ? a.part : (const double*)nullptr,
                       a.exact_l, a.exact_g, c.host_res, c.seq, c.pick, p.floor.f);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  if (Nc > 0) {
    hipLaunchKernelGGL(kde_batch_min_kernel, grid, dim3(256), 0, s, a.list, a.count, sg, a.exact_l, a.exact_g, a.best,
                       p.floor.f);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(kde_batch_key_kernel, grid, dim3(256), 0, s, a.list, a.count, sg, a.exact_l, a.exact_g, a.best,
                       a.key, p.floor.f);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(kde_batch_near_kernel, grid, dim3(256), 0, s, a.list, a.count, sg, a.exact_l, a.exact_g, a.key,
                       p.Pg(), p.Pb(), a.el, a.eg, a.near, a.segnear, p.floor.f);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(kde_batch_final_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, a.key, a.segcnt,
                       a.flags, a.segnear, a.list, a.exact_l, a.exact_g, p.Pg(), p.Pb(), a.el, a.eg, c.index_base,
                       batch_res, p.floor.f);
    HBX_LAUNCH_CHECK();
  }
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_workspace_bytes(int64_t Nc, int64_t nmax) { return (int64_t)ws_layout(Nc, nmax).total; }

int64_t hbx_kde_batch_workspace_bytes(int64_t Nc, int64_t seg, int64_t nmax) {
  if (seg < 1) return -1;
  return (int64_t)ws_layout(Nc, nmax, (Nc + seg - 1) / seg).total;
}

void* hbx_kde_result_ptr(void* workspace) { return (char*)workspace + ws_layout(0, 0).res; }

// One acquisition: score every candidate against l (good) and g (bad), shortlist, exact re-score,
// argmin.  index_base offsets the reported index (candidate sharding across GPUs).  The result
// (AcqResult) stays in the workspace; hbx_kde_result_ptr() gives its device address.
int hbx_kde_acquire(const double* cand, int64_t Nc, int64_t index_base, const void* pair, float* logl_out,
                    float* logg_out, void* workspace, int64_t ws_bytes, void* events, void* stream) {
  return acquire_impl(pair, {"hbx_kde_acquire", cand, Nc, Nc > 0 ? Nc : 1, index_base, logl_out, logg_out, nullptr,
                             workspace, ws_bytes, events, stream, nullptr, 0, PickOut{}});
}

// Batched acquisition: candidates [b*seg, min((b+1)*seg, Nc)) are the num_samples candidates of
// get_config call b; every segment gets its own exact argmin (index relative to the segment start,
// plus index_base) in results[b].  Same kernels as hbx_kde_acquire, one pass for all segments.
int hbx_kde_acquire_batch(const double* cand, int64_t Nc, int64_t seg, int64_t index_base, const void* pair,
                          float* logl_out, float* logg_out, void* results, void* workspace, int64_t ws_bytes,
                          void* stream) {
  if (!results) return hbx_fail(HBX_ERR_ARG, "hbx_kde_acquire_batch: null results");
  return acquire_impl(pair, {"hbx_kde_acquire_batch", cand, Nc, seg, index_base, logl_out, logg_out,
                             (AcqResult*)results, workspace, ws_bytes, nullptr, stream, nullptr, 0, PickOut{}});
}

void* hbx_kde_pair_bind(int32_t D, const void* params_good, const float* table_good, const double* X_good,
                        const int64_t* rows_good, int32_t variant_good, const void* params_bad,
                        const float* table_bad, const double* X_bad, const int64_t* rows_bad, int32_t variant_bad,
                        int32_t dc_pad, int32_t du_pad, int64_t nmax) {
  if (D <= 0 || D > HBX_MAX_D || !params_good || !params_bad || nmax < 0) {
    hbx_fail(HBX_ERR_ARG, "hbx_kde_pair_bind: bad arguments (D=%d, nmax=%lld)", D, (long long)nmax);
    return nullptr;
  }
  KdePairRef* b = new (std::nothrow) KdePairRef{D, params_good, table_good, X_good, rows_good, variant_good,
                                                params_bad, table_bad, X_bad, rows_bad, variant_bad, dc_pad,
                                                du_pad, nmax, hbx_score_floor(HBX_PDF_FLOOR_DEFAULT)};
  if (!b) hbx_fail(HBX_ERR_ARG, "hbx_kde_pair_bind: out of host memory");
  return b;
}

void hbx_kde_pair_free(void* pair) { delete (KdePairRef*)pair; }

// The pair's selection rules: every later acquisition on the handle forms its scores with rules->pdf_floor
// (min_bandwidth belongs to the fits and is only range-checked here).  NULL: the reference snapshot's.
int hbx_kde_pair_set_rules(void* pair, const hbx_rules* rules) {
  if (!pair) return hbx_fail(HBX_ERR_ARG, "hbx_kde_pair_set_rules: null pair");
  const int rc = hbx_rules_check("hbx_kde_pair_set_rules", rules);
  if (rc) return rc;
  ((KdePairRef*)pair)->floor = hbx_score_floor(rules ? rules->pdf_floor : HBX_PDF_FLOOR_DEFAULT);
  return HBX_OK;
}

// The drop-in's synchronous acquisition on a bound pair: the final kernel stores the 48-byte record into this
// thread's mapped host buffer as tagged words; the call spins until they carry its sequence number and copies the
// record to rec_out -- the acquisition and its pick on the host in one call, no copy kernel, no blocking
// synchronisation.
// err (nullable, device u8[Nc]: the GPU sampler's domain-error flags) sets HBX_ACQ_DOMAIN_ERR in the record
// when any is set; row_out (nullable, host f64[D]) receives the winning candidate's row -- both published by
// the same final kernel with the record (one wait for the draws' check, the pick and its row).
int hbx_kde_acquire_bound(const void* pair, const double* cand, int64_t Nc, int64_t index_base, void* workspace,
                          int64_t ws_bytes, const uint8_t* err, void* events, void* stream, void* rec_out,
                          double* row_out) {
  const char* who = "hbx_kde_acquire_bound";
  if (!pair || !rec_out || Nc < 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_acquire_bound: bad arguments");
  const KdePairRef& b = *(const KdePairRef*)pair;
  MappedBuf* mb = nullptr;
  int rc = hbx_mapped_acq(&mb);
  if (rc) return rc;
  char* pub = mb->p + PUB_OFF;
  const int32_t seq = mb->seq;
  const hipStream_t s = (hipStream_t)stream;
  const bool pick = err || row_out;  // (8 (13 + 2 D) <= PUB_BYTES for D <= HBX_MAX_D)
  rc = acquire_impl(pair, {who, cand, Nc, Nc > 0 ? Nc : 1, index_base, nullptr, nullptr, nullptr, workspace, ws_bytes,
                           events, stream, pick ? nullptr : (AcqResult*)pub, seq,
                           pick ? PickOut{cand, err, Nc, b.D, pub} : PickOut{}});
  if (rc) return rc;
  // the final kernel's tagged words: the record, then (a pick) the flag, then the row when there is a winner
  constexpr int RW = (int)(sizeof(AcqResult) / 4);
  constexpr int64_t SPIN = 20000000;  // ~0.1 s
  const volatile uint64_t* w = (const volatile uint64_t*)pub;
  uint32_t words[RW];
  rc = wait_tagged(w, RW, seq, words, s, SPIN, who);
  if (rc) return rc;
  AcqResult r;
  memcpy(&r, words, sizeof(AcqResult));
  if (pick) {
    uint32_t e = 0;
    rc = wait_tagged(w + RW, 1, seq, &e, s, SPIN, who);
    if (rc) return rc;
    if (e) r.flags |= HBX_ACQ_DOMAIN_ERR;
    if (row_out && r.index >= 0 && r.index - index_base < Nc) {
      rc = wait_tagged(w + RW + 1, 2 * b.D, seq, (uint32_t*)row_out, s, SPIN, who);
      if (rc) return rc;
    }
  }
  memcpy(rec_out, &r, sizeof(AcqResult));
  return HBX_OK;
}

// Byte offsets inside an acquisition workspace of (Nc, seg, nmax) -- hbx_kde_acquire: seg = Nc -- of
// what a host re-resolution of a near tie reads: out[0] shortlist count (i32), [1] shortlist (i32
// candidate indices), [2] near list (hbx_kde_acquire: the near set's candidate indices, res.near of
// them; batched: a 0/1 flag per shortlist entry), [3] exact l, [4] exact g (f64 per shortlist entry).
int hbx_kde_ws_offsets(int64_t Nc, int64_t seg, int64_t nmax, int64_t* out) {
  if (!out || seg < 1) return hbx_fail(HBX_ERR_ARG, "hbx_kde_ws_offsets: bad arguments");
  const WsLayout w = ws_layout(Nc, nmax, seg >= Nc ? 1 : (Nc + seg - 1) / seg);
  out[0] = (int64_t)w.count;
  out[1] = (int64_t)w.list;
  out[2] = (int64_t)w.near;
  out[3] = (int64_t)w.exact_l;
  out[4] = (int64_t)w.exact_g;
  return HBX_OK;
}

}  // extern "C"

