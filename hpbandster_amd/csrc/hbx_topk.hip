// hbx_topk.hip -- top-k acquisition on MI355X (gfx950): the k best candidates of ONE pool, ranked exactly.
//
// hbx_kde_acquire answers "which candidate minimises s = max(f, g) / max(l, f)" (bohb.py:149-152; f: the pair's
// score floor, 1e-8 unless set);
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
// Staged scoring (hbx_topk_staged; where acq_staged_supported(plan) holds and HBX_STAGED says so with the argmin's
// meaning -- 0 never, 2 wherever supported, unset from Nc x nmax >= HBX_STAGED_TOPK_MIN_PAIRS, hbx_acquire.h): g
// only for the candidates that can still rank.  score_i >= f / max(l_i, f)
// whatever g is (hbx_staged.hip), with the k-th place in the role of the best.  All on the caller's stream:
//   1 score l      hbx_staged.hip's stage 1 as it is (staged_score_l): the good KDE's coarse pair kernel, then
//                  staged_l_kernel -- rescue, split merge, [llo, lhi], lhi kept in a.lo -- which here also writes
//                  every candidate's ordered key of -llo
//     L_(k+1)      the (k+1)-th largest llo: the radix select below (topk_hist x4) over those keys, resolved by
//                  topk_lthr into the state words.  Fewer than k+1 finite llo: -inf, no threshold
//   2 seeds        staged_seed_kernel: lhi >= L_(k+1) - ln 4, up to the list's capacity (4096 > k + 1); the rest
//                  fall through to 4.  Any subset of the band would do, and the list's order is free
//   3 score seeds  the bad KDE's list instance and staged_merge_kernel, then topk_useed (one block): U_(k+1)_seed,
//                  the (k+1)-th smallest upper score bound over the seeds; +inf with fewer than k+1 finite ones and
//                  under the bad KDE's overflow guard (log_norm + ln n within 100 of 700)
//   4 survivors    staged_survivor_kernel: every unseeded candidate with C - max(lhi, C) <= U_(k+1)_seed ('<=':
//                  ties survive), scored like the argmin's (split up to the capacity, unsplit beyond); every
//                  unseeded candidate's a.lo becomes that l-only bound, lhi > 700 raises the overflow flag
//   5 select       over the evaluated candidates (seeds, survivors) only: topk_staged_bounds (the survivors'
//                  partials merged, marked g estimates re-scored, then topk_bounds' arithmetic, the key of hi per
//                  list entry), topk_hist x4 and topk_shortlist over the list's entries -- U_k, the k-th smallest
//                  finite hi among them, and {lo <= U_k}.  Under the overflow flag the shortlist is every candidate
//                  whose lo is not NaN, pruned ones included, as in the unstaged call.
//   then acq_exact and topk_final, unchanged.
// Why the result is the unstaged one.  A pruned candidate's true score is >= f / max(l, f) >= exp(its
// l-only bound) > exp(U_(k+1)_seed).  U_(k+1)_seed is at least the (k+1)-th smallest true score, because k+1
// seeds have a true score <= it.  So a pruned candidate lies strictly behind k+1 others, ties by index included:
// it is neither returned nor the best excluded entry the near-tie test reads, and with lo > U_(k+1)_seed >= U_k
// (the evaluated candidates hold those k+1 seeds) and hi = +inf it would enter neither the select nor the
// shortlist.  Everything returned comes from exact fp64 scores of a shortlist that holds the true top k+1 (the
// argument above, over the evaluated candidates).  So count, flags and every record's index, score, pdf_l, pdf_g
// and rel (staged pairs are unsigned: rel reads no g estimate) are the unstaged call's; the header's `shortlist`
// may differ, because the evaluated candidates' fp32 estimates come from launches with other observation splits
// and move within their bounds.  (HBX_ACQ_OVERFLOW from a pruned candidate's g: the guard, as in hbx_staged.hip.)
// The one regime that does not prune: with fewer than k+1 candidates that certainly score below 1,
// U_(k+1)_seed >= 0 and every candidate with l below the clamp survives (bound 0); the call then costs the
// unstaged one plus the selection launches.
//
// Result block (hbx_kde_topk_result_bytes(k) = 16 + 40 k bytes, include/hbx.h):
//   header {i32 count, i32 shortlist, i32 flags, i32 k}, then `count` records of 40 bytes
//   {i64 index, f64 score, f64 pdf_l, f64 pdf_g, f32 rel, i32 0}
#include "hbx_acq_impl.h"
#include "hbx_acquire.h"
#include "hbx_rescue_impl.h"
#include "hbx_topk_rank.h"

#define TOPK_KEY_INF 0xFF800000u  // hbx_f2ord(+inf): keys below it are finite upper bounds
#define TOPK_HIST_WORDS (4 * 256)  // workspace of the k-th bound's radix select: 4 histograms of 256 bins

__global__ __launch_bounds__(256) void topk_bounds_kernel(const KdeEst* __restrict__ el,
                                                          const KdeEst* __restrict__ eg, int64_t Nc,
                                                          float* __restrict__ lo, uint32_t* __restrict__ hik,
                                                          int32_t* __restrict__ flags, uint32_t* __restrict__ hist,
                                                          ScoreFloor F) {
  if (blockIdx.x == 0)  // the select's histograms (its passes are later launches)
    for (int j = threadIdx.x; j < TOPK_HIST_WORDS; j += 256) hist[j] = 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool of = false;
  if (i < Nc) {
    const ScoreIv v = score_interval(el[i], eg[i], F);
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

// Entries of a staged call's evaluated list (seeds first, then survivors) from its state words; null: every one of
// the Nc candidates (the unstaged call)
__device__ __forceinline__ int64_t topk_entries(const uint32_t* __restrict__ stage, int32_t cap, int64_t Nc) {
  if (!stage) return Nc;
  const int64_t ns = (int64_t)stage[HBX_ST_NSEED] < cap ? (int64_t)stage[HBX_ST_NSEED] : cap;
  const int64_t n = ns + (int64_t)stage[HBX_ST_NSURV];
  return n < Nc ? n : Nc;
}

#define TOPK_HIST_PER_BLOCK 4096  // keys per block of a select pass
// (stage non-null: the keys are the evaluated list's, one per entry; blocks past its end exit at once)
__global__ __launch_bounds__(256) void topk_hist_kernel(const uint32_t* __restrict__ hik, int64_t Nc, int32_t k,
                                                        int pass, uint32_t* __restrict__ hist,
                                                        const uint32_t* __restrict__ stage, int32_t cap) {
  __shared__ uint32_t h[256];
  Nc = topk_entries(stage, cap, Nc);
  if ((int64_t)blockIdx.x * TOPK_HIST_PER_BLOCK >= Nc) return;  // uniform
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
// The evaluated list of a staged call (hbx_staged.hip; all null / 0: the unstaged call, every candidate)
struct TopkEval {
  const uint32_t* stage;
  const int32_t* seeds;
  const int32_t* surv;
  int32_t cap;
};
__device__ __forceinline__ int32_t topk_entry(const TopkEval& ev, int64_t e) {
  const int64_t ns = (int64_t)ev.stage[HBX_ST_NSEED] < ev.cap ? (int64_t)ev.stage[HBX_ST_NSEED] : ev.cap;
  return e < ns ? ev.seeds[e] : ev.surv[e - ns];
}

// (ev.stage non-null: over the evaluated list's entries instead of all candidates -- a pruned candidate has
// lo > U_k -- unless the overflow flag asks for every candidate whose lo is not NaN)
__global__ __launch_bounds__(256) void topk_shortlist_kernel(const float* __restrict__ lo, int64_t Nc, int32_t k,
                                                             const uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ U,
                                                             const int32_t* __restrict__ flags,
                                                             int32_t* __restrict__ list, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ rescue_cnt, TopkEval ev) {
  const bool listed = ev.stage != nullptr && (flags[0] & 1) == 0;
  if (listed) Nc = topk_entries(ev.stage, ev.cap, Nc);
  if (blockIdx.x != 0 && (int64_t)blockIdx.x * TOPK_SHORT_PER_BLOCK >= Nc) return;  // uniform
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
    const int64_t e = b0 + r * 256 + threadIdx.x;
    int64_t i = e;
    bool in = false;
    if (e < Nc) {
      if (listed) i = topk_entry(ev, e);
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
// the staged top-k's own steps (file header, "Staged scoring"); the launches between them are hbx_staged.hip's

// One block behind the select over the keys of -llo: the seed band's reference L_(k+1), the (k+1)-th largest llo,
// into the state words' Lmax (where the seed kernel reads the argmin's largest llo); fewer than k+1 finite llo:
// -inf, every candidate with an l is a seed.  The histograms are zeroed again for the select of U_k.
__global__ __launch_bounds__(256) void topk_lthr_kernel(uint32_t* __restrict__ hist, int32_t k1,
                                                        uint32_t* __restrict__ stage) {
  const TopkSel sel = topk_resolve(hist, k1, 4);  // (ends with a barrier: every read of hist is done)
  if (threadIdx.x == 0)
    stage[HBX_ST_LMAX] = sel.rank == 0xffffffffu ? hbx_f2ord(-INFINITY) : hbx_f2ord(-hbx_ord2f(sel.prefix));
  for (int j = threadIdx.x; j < TOPK_HIST_WORDS; j += 256) hist[j] = 0;
}

// One block behind the seeds' merge: U_(k+1)_seed, the (k+1)-th smallest upper score bound over the seed list (at
// most STAGED_LIST_CAP entries, their ordered keys in registers: topk_hist's radix select with the histogram in
// LDS and one wave scanning its 256 bins), into the state words' U_seed.  A seed whose g estimate is the rescue
// marker counts as +inf here (the bounds kernel re-scores it).  +inf as well with fewer than k+1 finite bounds,
// and under the bad KDE's overflow guard (staged_merge_kernel's test).
#define TOPK_USEED_T 1024
#define TOPK_USEED_PT (STAGED_LIST_CAP / TOPK_USEED_T)
static_assert(HBX_TOPK_MAX_K < STAGED_LIST_CAP, "a full seed list holds k + 1 seeds");
__global__ __launch_bounds__(TOPK_USEED_T) void topk_useed_kernel(const int32_t* __restrict__ seeds, int32_t cap,
                                                                  const KdeEst* __restrict__ el,
                                                                  const KdeEst* __restrict__ eg,
                                                                  const KdeParams* __restrict__ Pb, int32_t k,
                                                                  uint32_t* __restrict__ stage, ScoreFloor F) {
  __shared__ uint32_t hb[256];
  __shared__ uint32_t s_prefix, s_rank;
  const int t = threadIdx.x;
  int32_t nseed = (int32_t)stage[HBX_ST_NSEED];
  if (nseed > cap) nseed = cap;
  uint32_t key[TOPK_USEED_PT];
#pragma unroll
  for (int r = 0; r < TOPK_USEED_PT; ++r) {
    const int j = r * TOPK_USEED_T + t;
    key[r] = TOPK_KEY_INF;
    if (j < nseed) {
      const int32_t i = seeds[j];
      const KdeEst b = eg[i];
      if (b.err != -1.f) {
        const ScoreIv v = score_interval(el[i], b, F);
        if (!v.lnan && v.shi == v.shi) key[r] = hbx_f2ord(v.shi);
      }
    }
  }
  if (t == 0) {
    s_prefix = 0;
    s_rank = (uint32_t)k + 1;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    if (t < 256) hb[t] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix, rank = s_rank;
    if (rank == 0xffffffffu) break;  // uniform: fewer than k+1 finite keys
#pragma unroll
    for (int r = 0; r < TOPK_USEED_PT; ++r)
      if (key[r] < TOPK_KEY_INF && ((key[r] ^ prefix) & himask) == 0) atomicAdd(&hb[(key[r] >> shift) & 255u], 1u);
    __syncthreads();
    if (t < 64) {  // one wave: lane t owns bins 4 t .. 4 t + 3
      uint32_t c[4], sum = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        c[q] = hb[4 * t + q];
        sum += c[q];
      }
      uint32_t incl = sum;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (t >= o) incl += v;
      }
      uint32_t run = incl - sum;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (run < rank && rank <= run + c[q]) {
          s_prefix = prefix | ((uint32_t)(4 * t + q) << shift);
          s_rank = rank - run;
        }
        run += c[q];
      }
      if (t == 63 && incl < rank) s_rank = 0xffffffffu;  // (first pass only: its total counts every finite key)
    }
    __syncthreads();
  }
  if (t == 0) {
    const bool guard = Pb->lnpdf_guard != 0;  // log_norm + ln n < 600 (hbx_prep.hip)
    stage[HBX_ST_USEED] = guard && s_rank != 0xffffffffu ? s_prefix : TOPK_KEY_INF;
  }
}

// The bounds pass over the evaluated candidates only (entry e of seeds-then-survivors; a block owns 1024 consecutive
// entries, blocks past the last one exit): the survivors' split partials merged and scattered (the seeds' merge has
// run; an unsplit survivor launch scattered its own), marked g estimates re-scored, then topk_bounds_kernel's
// arithmetic: lo[i], and the upper bound's key into ekey[e] -- per entry, for the select of U_k.  Every other
// candidate's lo is the l-only bound the survivor pass wrote.
struct TopkStagedArgs {
  const KdeEst* part;  // the survivor launch's split partials [ns][cap]
  int32_t cap, ns;
  TopkEval ev;
  int64_t Nc;
  const double* cand;
  int32_t D;
  const KdeParams* Pb;
  const KdeEst* el;
  KdeEst* eg;
  float* lo;
  uint32_t* ekey;
  int32_t* flags;
  const int32_t* rescue_cnt;
  ScoreFloor F;
};
__global__ __launch_bounds__(256) void topk_staged_bounds_kernel(TopkStagedArgs t) {
  int64_t nseed = (int32_t)t.ev.stage[HBX_ST_NSEED], nsurv = (int32_t)t.ev.stage[HBX_ST_NSURV];
  if (nseed > t.cap) nseed = t.cap;
  if (nsurv > t.Nc) nsurv = t.Nc;
  const bool split = nsurv <= t.cap;  // else the unsplit launch scattered its estimates itself
  const int64_t total = nseed + nsurv < t.Nc ? nseed + nsurv : t.Nc;
  if ((int64_t)blockIdx.x * 1024 >= total) return;
  const int32_t nres = *t.rescue_cnt;  // markers counted by the scoring launches (a hint, as in the combine)
  bool of = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t e = (int64_t)blockIdx.x * 1024 + r * 256 + threadIdx.x;
    if (e >= total) continue;
    const int64_t i = e < nseed ? t.ev.seeds[e] : t.ev.surv[e - nseed];
    KdeEst b;
    bool store = false;
    if (e < nseed || !split) {
      b = t.eg[i];
    } else {
      const int64_t ks = e - nseed;
      bool mark = false;
      for (int q = 0; q < t.ns; ++q) mark = mark || t.part[(int64_t)q * t.cap + ks].err == -1.f;
      b = {0.f, -INFINITY, -1.f, 0.f};
      if (!mark) b = merge_splits(t.part, t.cap, ks, t.ns);
      store = true;
    }
    if (nres != 0 && b.err == -1.f) {  // rare
      b = kde_rescue_one<0, false, true>(t.cand, i, t.D, t.Pb);
      store = true;
    }
    if (store) t.eg[i] = b;
    const ScoreIv v = score_interval(t.el[i], b, t.F);
    of = of || v.of;
    t.lo[i] = v.lnan ? NAN : (v.slo == v.slo ? v.slo : -INFINITY);
    t.ekey[e] = hbx_f2ord((v.lnan || v.shi != v.shi) ? INFINITY : v.shi);
  }
  if (__ballot(of) != 0 && (threadIdx.x & 63) == 0) atomicOr(t.flags, HBX_ACQ_OVERFLOW);  // rare
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
    const KdeEst* __restrict__ eg, TopkHead* __restrict__ head, TopkRec* __restrict__ rec, double pfloor) {
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
      const double s = bohb_score(exact_g[p], exact_l[p], pfloor);
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
                    uint32_t* hist, const ScoreFloor& F, hipStream_t s) {
  hipLaunchKernelGGL(topk_bounds_kernel, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, el, eg, Nc, lo, hik,
                     flags, hist, F);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// U[0] = the k-th smallest finite hi (+inf with fewer than k), then the shortlist {i: lo[i] == lo[i] &&
// (flags[0] & 1 || lo[i] <= U[0])} into list / count; zeroes the scoring launch's marker count
// ev (a staged call): hik holds one key per entry of the evaluated list, and the shortlist comes from that list
static int hbx_topk_shortlist(const float* lo, const uint32_t* hik, int64_t Nc, int32_t k, uint32_t* hist, uint32_t* U,
                       const int32_t* flags, int32_t* list, int32_t* count, int32_t* rescue_cnt, const TopkEval& ev,
                       hipStream_t s) {
  if (hik) {  // the radix select (no keys: an exact-only acquisition, its histograms zero, U_k = +inf)
    const unsigned gh = (unsigned)((Nc + TOPK_HIST_PER_BLOCK - 1) / TOPK_HIST_PER_BLOCK);
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(topk_hist_kernel, dim3(gh), dim3(256), 0, s, hik, Nc, k, pass, hist, ev.stage, ev.cap);
      HBX_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(topk_shortlist_kernel, dim3((unsigned)((Nc + TOPK_SHORT_PER_BLOCK - 1) / TOPK_SHORT_PER_BLOCK)),
                     dim3(256), 0, s, lo, Nc, k, (const uint32_t*)hist, U, flags, list, count, rescue_cnt, ev);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// the k smallest (score, index) of the re-scored shortlist, ranked, into the result block
static int hbx_topk_final(const int32_t* list, const int32_t* count, const double* exact_l, const double* exact_g,
                   const int32_t* flags, int64_t index_base, int32_t k, const KdeParams* Pg, const KdeParams* Pb,
                   const KdeEst* el, const KdeEst* eg, void* results, double pfloor, hipStream_t s) {
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "top-k: k=%d outside [1, %d]", k, HBX_TOPK_MAX_K);
  hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(TOPK_T), 0, s, list, count, exact_l, exact_g, flags,
                     index_base, k, Pg, Pb, el, eg, (TopkHead*)results, (TopkRec*)((char*)results + sizeof(TopkHead)),
                     pfloor);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// The staged top-k's scoring and selection (file header, "Staged scoring"): afterwards a.el holds every candidate's
// l estimate, a.eg the evaluated candidates' g estimates, a.list / a.count the shortlist, a.flags the overflow
// rule, the state words the counts -- what acq_exact and the final ranking read.
static int hbx_topk_staged(const AcqPlan& plan, const KdePairRef& p, const double* cand, int64_t Nc, int32_t k,
                           const AcqWs& a, uint32_t* keys, uint32_t* hist, hipStream_t s) {
  // 1: l for every candidate, the keys of -llo, the histograms zeroed
  int rc = staged_score_l(plan, p, cand, Nc, a, nullptr, s, keys, hist, TOPK_HIST_WORDS);
  if (rc) return rc;
  // L_(k+1) into the state words (and the histograms zeroed again)
  const unsigned gh = (unsigned)((Nc + TOPK_HIST_PER_BLOCK - 1) / TOPK_HIST_PER_BLOCK);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(topk_hist_kernel, dim3(gh), dim3(256), 0, s, (const uint32_t*)keys, Nc, k + 1, pass, hist,
                       (const uint32_t*)nullptr, 0);
    HBX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(topk_lthr_kernel, dim3(1), dim3(256), 0, s, hist, k + 1, a.stage);
  HBX_LAUNCH_CHECK();
  // 2, 3: the seeds and their g; U_(k+1)_seed
  rc = staged_score_seeds(plan, p, cand, Nc, a, s, false, false);
  if (rc) return rc;
  const int32_t cap = a.list_cap;
  hipLaunchKernelGGL(topk_useed_kernel, dim3(1), dim3(TOPK_USEED_T), 0, s, (const int32_t*)a.seeds, cap,
                     (const KdeEst*)a.el, (const KdeEst*)a.eg, p.Pb(), k, a.stage, p.floor);
  HBX_LAUNCH_CHECK();
  // 4: the survivors and their g; every unseeded candidate's l-only bound into a.lo
  rc = staged_score_survivors(plan, p, cand, Nc, a, s, true);
  if (rc) return rc;
  // 5: bounds, U_k and the shortlist over the evaluated candidates
  const TopkEval ev{a.stage, a.seeds, a.surv, cap};
  const TopkStagedArgs ta{a.lpart, cap, (int32_t)list_splits(p.nmax), ev, Nc, cand, p.D, p.Pb(), a.el, a.eg, a.lo,
                          keys, a.flags, a.rescue, p.floor};
  hipLaunchKernelGGL(topk_staged_bounds_kernel, dim3((unsigned)((Nc + 1023) / 1024)), dim3(256), 0, s, ta);
  HBX_LAUNCH_CHECK();
  return hbx_topk_shortlist(a.lo, keys, Nc, k, hist, a.U, a.flags, a.list, a.count, a.rescue, ev, s);
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
  const WsLayout w = ws_layout(Nc, p.nmax);
  if (Nc == 0) {  // count = 0 and no launch: a zeroed header, and "did not stage" for hbx_kde_acquire_stats
    HBX_HIP(hipMemsetAsync(results, 0, 16, s));
    HBX_HIP(hipMemsetAsync((char*)workspace + w.stage, 0, 4 * HBX_ST_WORDS, s));
    return HBX_OK;
  }
  AcqPlan plan;
  rc = acq_plan(p, true, &plan);
  if (rc) return rc;
  const AcqWs a(workspace, w);
  uint32_t* hik = (uint32_t*)a.near;                         // the upper bounds' keys in the near list's place
  uint32_t* hist = (uint32_t*)((char*)workspace + w.total);  // the select's histograms after the argmin's workspace
  // Staged scoring (file header): the argmin's switch with the same meaning, the top-k's own size threshold
  const int stg = hbx_staged_mode();
  if (stg && acq_staged_supported(plan) && (stg == 2 || (double)Nc * (double)p.nmax >= HBX_STAGED_TOPK_MIN_PAIRS)) {
    rc = hbx_topk_staged(plan, p, cand, Nc, k, a, hik, hist, s);
    if (rc) return rc;
    rc = acq_exact(p, cand, Nc, a, false, true, s);
    if (rc) return rc;
    return hbx_topk_final(a.list, a.count, a.exact_l, a.exact_g, a.flags, index_base, k, p.Pg(), p.Pb(), a.el, a.eg,
                          results, p.floor.f, s);
  }
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
    rc = hbx_topk_bounds(a.el, a.eg, Nc, a.lo, hik, a.flags, hist, p.floor, s);
    if (rc) return rc;
  }
  rc = hbx_topk_shortlist(a.lo, plan.exact_only ? nullptr : hik, Nc, k, hist, a.U, a.flags, a.list, a.count, a.rescue,
                          TopkEval{}, s);
  if (rc) return rc;
  rc = acq_exact(p, cand, Nc, a, false, true, s);
  if (rc) return rc;
  return hbx_topk_final(a.list, a.count, a.exact_l, a.exact_g, a.flags, index_base, k, p.Pg(), p.Pb(), a.el, a.eg,
                        results, p.floor.f, s);
}

}  // extern "C"
