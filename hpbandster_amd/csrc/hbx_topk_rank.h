// hbx_topk_rank.h -- the running best-(k+1) by (score bits, index) over a stream of any length, one block, LDS.
// Users: topk_final_kernel (hbx_topk.hip: the single pool's ranking) and groups_topk_kernel (hbx_groups.hip: one
// block per group).  Both feed it chunks of at most T entries, one per thread, and read the ranked entries back.
//
// Entries are (score bits, candidate index, payload position); what a position refers to (the caller's exact pdfs,
// its error bound) stays where the caller keeps it.  [0, nb) are the best so far in ascending (score, index) order,
// [nb, nb + pend) accepted since the last merge, unordered.  When a chunk no longer fits behind them the array is
// sorted (bitonic, padded to a power of two) and cut to `keep`; from then on the keep-th best is a threshold and
// entries not below it are dropped before they are stored.  Scores are positive and never NaN here (the caller
// drops NaN), so their bits order like the scores; the index breaks ties, so the order is total and the result
// does not depend on the order of arrival or on thread timing.
#pragma once
#include <stdint.h>

// the result block both calls write (include/hbx.h: hbx_kde_acquire_topk)
struct TopkHead {
  int32_t count, shortlist, flags, k;
};
struct TopkRec {
  int64_t index;
  double score, pdf_l, pdf_g;
  float rel;
  int32_t pad;
};
static_assert(sizeof(TopkHead) == 16 && sizeof(TopkRec) == 40, "the documented result block layout");

__device__ __forceinline__ bool topk_less(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// T: threads of the block (a multiple of 64), every one of which calls push / merge / finish together.
// cap: entries of each LDS array, a power of two with keep + T <= cap (a chunk fits behind the kept entries).
template <int T>
struct TopkRank {
  uint64_t* sk;  // LDS [cap]
  int32_t* si;   // LDS [cap]
  int32_t* sp;   // LDS [cap]
  int32_t* swc;  // LDS [T / 64]
  int cap, keep;
  int nb, pend;  // uniform
  // only entries below the keep-th best so far can still enter (everything, until that many are held)
  uint64_t tkey;
  int32_t tidx;

  __device__ void init(uint64_t* sk_, int32_t* si_, int32_t* sp_, int32_t* swc_, int cap_, int keep_) {
    sk = sk_;
    si = si_;
    sp = sp_;
    swc = swc_;
    cap = cap_;
    keep = keep_;
    nb = pend = 0;
    tkey = ~0ull;
    tidx = INT32_MAX;
  }

  __device__ bool enters(uint64_t key, int32_t idx) const { return topk_less(key, idx, tkey, tidx); }

  __device__ void merge() {  // whole block, uniform: sort [0, nb + pend), keep the first `keep`
    const int t = threadIdx.x;
    const int n = nb + pend;
    int W = 2;
    while (W < n) W <<= 1;
    for (int j = n + t; j < W; j += T) {  // padding sorts last (no score has these bits: a NaN's)
      sk[j] = ~0ull;
      si[j] = INT32_MAX;
      sp[j] = -1;
    }
    for (int size = 2; size <= W; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        __syncthreads();
        for (int pr = t; pr < W / 2; pr += T) {
          const int i = 2 * pr - (pr & (stride - 1)), j = i + stride;
          const bool asc = (i & size) == 0;
          const uint64_t ka = sk[i], kb = sk[j];
          const int32_t ia = si[i], ib = si[j];
          if (asc ? topk_less(kb, ib, ka, ia) : topk_less(ka, ia, kb, ib)) {
            sk[i] = kb;
            sk[j] = ka;
            si[i] = ib;
            si[j] = ia;
            const int32_t pa = sp[i];
            sp[i] = sp[j];
            sp[j] = pa;
          }
        }
      }
    }
    __syncthreads();
    nb = n < keep ? n : keep;
    pend = 0;
    if (nb == keep) {
      tkey = sk[keep - 1];
      tidx = si[keep - 1];
    }
    __syncthreads();  // (the threshold is read before anything is appended behind the kept entries)
  }

  // one chunk: this thread's entry (acc: it is rankable and enters()), appended in thread order
  __device__ void push(bool acc, uint64_t key, int32_t idx, int32_t p) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint64_t b = __ballot(acc);
    if (lane == 0) swc[wv] = (int32_t)__popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
      off += w < wv ? swc[w] : 0;
      tot += swc[w];
    }
    if (nb + pend + tot > cap) merge();  // uniform; afterwards nb <= keep and pend = 0: the chunk fits
    if (acc) {
      const int at = nb + pend + off + (int)__popcll(b & ((1ull << lane) - 1));
      sk[at] = key;
      si[at] = idx;
      sp[at] = p;
    }
    pend += tot;
    __syncthreads();
  }

  __device__ void finish() {  // afterwards [0, nb) is ranked, nb <= keep
    if (nb + pend > 0) merge();
  }
};
