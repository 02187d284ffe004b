// hbx_groups_rank.hip -- grouped log-ratio ranking: per bracket the k candidates with the smallest s = ln g - ln l,
// ordered by (s, index), with no floor (hbx_kde_rank_groups), and the composite call that forms both ln-pdfs first
// (hbx_kde_rank_logratio_groups: hbx_kde_logpdf_groups for both KDEs, then the ranking, one stream, one workspace).
// The floored score max(f, g) / max(l, f) is exactly 1 wherever both densities lie under f (bohb.py:124-169 at
// config #5's dims); ln g - ln l still tells such candidates apart.
//
// The order (include/hbx.h): a candidate's key is hbx_d2ord(s) -- finite and -inf values by value, -0 as +0, then
// +inf, every NaN past +inf; NaN keys are never ranked or counted, equal keys rank by lower index.  (key, index) is a
// total order, so the result does not depend on the order of arrival or on thread timing: two runs give the same bytes.
//
// groups_rank_kernel<KMAX, NW, LIST, PART>, one block of 64 NW threads per (group, part).  A block walks its range two
// candidates per lane and step: one 16-byte load from each ln array where both rows share their 16-byte phase (a
// row of odd C starts 8 bytes off: the range is then entered one position early and the dead position masked), two
// 8-byte loads at the range's ends and where the phases differ.  Every candidate is read once.
//
//   KMAX = 64   the best list is one (key, index) per lane of a wave, ascending by lane.  The wave's threshold is lane
//               k - 1's entry; a step with no entrant costs the loads, one compare per candidate and a ballot.
//               Otherwise the step's entrants (the other lanes padded) are sorted across the wave -- a bitonic network
//               of 21 exchanges by lane shuffles -- and merged into the list: min(list[i], batch[63 - i]) is bitonic
//               and holds the 64 smallest, 6 more exchanges order it.  The NW waves take the steps in turn, meet at the
//               block's only barrier, and wave 0 merges the lists from LDS the same way.  NW = 1 serves pools of at most
//               256 candidates (config #5's 64: a block is one wave, nothing is idle), NW = 4 longer ones.
//   KMAX = 1024 the best list lives in LDS: hbx_topk_rank.h's arrays and its bitonic merge (cap 2048, keep k; the payload
//               column is unused).  Appending is this kernel's own: entrants are staged behind the list by a wave-level
//               ballot and prefix count and one LDS atomic per wave, onto one of three rotating counters -- step c adds
//               to counter c % 3, reads the final count of step c - 1 and clears the counter of step c + 1, so a step
//               costs one barrier and every thread holds the same pending count.  When the next step (512 candidates)
//               could overflow the arrays the block merges, and TopkRank's threshold (the k-th best key and index) is
//               refreshed; a candidate that cannot enter costs one compare.
//
// Long pools are sliced (rank_parts: from 32768 candidates, slices of at least 16384, at most 64): a first launch
// (PART) leaves each slice's k best candidate indices in the workspace, -1 padded; a second (LIST) ranks each
// group's parts * k listed candidates, re-reading their two values.  Two launches on one stream: no spin-wait, no
// cross-block hand-off, no atomic to global memory.  Control flow around every barrier is block-uniform: the
// status test, the trip counts and the merge decision depend on block-uniform values only.
#include "hbx_common.h"
#include "hbx_topk_rank.h"

#define RANK_T 256
#define RANK_CAP 2048                         // LDS list: keep <= 1024 and a step of 2 * RANK_T behind it
#define RANK_KEY_PINF 0xFFF0000000000000ull   // hbx_d2ord(+inf): larger keys are NaN
#define RANK_BAD (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED)
#define RANK_SLICE_FROM 32768
#define RANK_SLICE_MIN 16384
#define RANK_PARTS_MAX 64

// the result block (include/hbx.h: hbx_kde_rank_groups)
struct RankHead {
  int32_t count, k, status, pad;
};
struct RankRec {
  int32_t index, pad;
  double score, ln_l, ln_g;
};
static_assert(sizeof(RankHead) == 16 && sizeof(RankRec) == 32 && HBX_RANK_BLOCK_BYTES(3) == 16 + 3 * 32,
              "the documented result block layout");
static_assert(HBX_RANK_MAX_K + 2 * RANK_T <= RANK_CAP, "a step fits behind the kept entries");

struct RankArgs {
  const double* ln_l;  // [B][C]
  const double* ln_g;
  const int32_t* status;  // [B]
  int64_t C;
  int32_t k;
  int32_t parts;   // slices per group (1: one launch)
  int64_t slice;   // candidates per slice
  int32_t* part;   // workspace [B][parts][k]: each slice's best candidate indices, -1 padded
  char* out;       // B result blocks
};

static int32_t rank_parts(int64_t C) {
  if (C < RANK_SLICE_FROM) return 1;
  const int64_t p = C / RANK_SLICE_MIN;
  return (int32_t)(p < RANK_PARTS_MAX ? p : RANK_PARTS_MAX);
}

// Positions p and p + 1 of the block's range [lo, hi): candidate p of the row, or (LIST) the candidate that entry p
// of the index list names.  A dead position gets the NaN key, which never enters.
template <bool LIST>
__device__ __forceinline__ void rank_fetch2(const double* __restrict__ rl, const double* __restrict__ rg,
                                            const int32_t* __restrict__ list, bool vec, int64_t p, int64_t lo,
                                            int64_t hi, uint64_t (&key)[2], int32_t (&idx)[2]) {
  key[0] = key[1] = ~0ull;
  idx[0] = idx[1] = INT32_MAX;
  if (!LIST && vec && p >= lo && p + 1 < hi) {  // (p is even past the row's 16-byte phase: both loads are aligned)
    const double2 l = *(const double2*)(rl + p), g = *(const double2*)(rg + p);
    key[0] = hbx_d2ord(g.x - l.x);
    key[1] = hbx_d2ord(g.y - l.y);
    idx[0] = (int32_t)p;
    idx[1] = (int32_t)p + 1;
    return;
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int64_t q = p + e;
    if (q < lo || q >= hi) continue;
    const int32_t i = LIST ? list[q] : (int32_t)q;
    if (i < 0) continue;
    key[e] = hbx_d2ord(rg[i] - rl[i]);
    idx[e] = i;
  }
}

// one exchange of a wave-wide network: the lane keeps the smaller (keep_min) or larger of its entry and lane ^ stride's
__device__ __forceinline__ void rank_cx(uint64_t& k, int32_t& i, int stride, bool keep_min) {
  const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)k, stride);
  const int32_t oi = __shfl_xor(i, stride);
  if (topk_less(ok, oi, k, i) == keep_min) {
    k = ok;
    i = oi;
  }
}

// any 64 entries, one per lane -> ascending by lane
__device__ __forceinline__ void rank_wave_sort(uint64_t& k, int32_t& i, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1)
      rank_cx(k, i, stride, ((lane & stride) == 0) == ((lane & size) == 0));
}

// two ascending lists, one entry per lane each -> the 64 smallest of both in (k, i), ascending by lane
__device__ __forceinline__ void rank_wave_merge(uint64_t& k, int32_t& i, uint64_t ck, int32_t ci, int lane) {
  const uint64_t rk = (uint64_t)__shfl((unsigned long long)ck, 63 - lane);
  const int32_t ri = __shfl(ci, 63 - lane);
  if (topk_less(rk, ri, k, i)) {
    k = rk;
    i = ri;
  }
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) rank_cx(k, i, stride, (lane & stride) == 0);
}

// entry j of a group's ranked list (idx < 0: past the count) to the slice's index list or to the result block
template <bool PART>
__device__ __forceinline__ void rank_emit(const RankArgs& A, const double* rl, const double* rg, int32_t* plist,
                                          RankRec* rec, int j, int32_t idx) {
  if (PART) {
    plist[j] = idx;
    return;
  }
  RankRec o;
  o.index = idx;
  o.pad = 0;
  o.score = o.ln_l = o.ln_g = __longlong_as_double(0x7FF8000000000000ll);
  if (idx >= 0) {
    o.ln_l = rl[idx];
    o.ln_g = rg[idx];
    o.score = o.ln_g - o.ln_l;  // (the value the key was formed from, -0 kept)
  }
  rec[j] = o;
}

template <int KMAX, int NW, bool LIST, bool PART>
__global__ __launch_bounds__(64 * NW) void groups_rank_kernel(RankArgs A) {
  static_assert(KMAX == 64 || (KMAX == HBX_RANK_MAX_K && NW * 64 == RANK_T), "the two instances by k");
  constexpr int T = 64 * NW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = A.k;
  const int64_t b = PART ? (int64_t)blockIdx.x / A.parts : (int64_t)blockIdx.x;
  const int part = PART ? (int)((int64_t)blockIdx.x - b * A.parts) : 0;
  const double* rl = A.ln_l + b * A.C;
  const double* rg = A.ln_g + b * A.C;
  int32_t* plist = PART ? A.part + ((int64_t)blockIdx.x) * k : nullptr;
  const int32_t* list = LIST ? A.part + b * A.parts * (int64_t)k : nullptr;
  RankHead* head = (RankHead*)(A.out + b * (int64_t)HBX_RANK_BLOCK_BYTES(k));
  RankRec* rec = (RankRec*)(head + 1);
  const int st = A.status[b];
  if (st & RANK_BAD) {  // uniform: no model, nothing is ranked (a LIST launch does not read the group's lists)
    if (!PART) {
      for (int j = tid; j < k; j += T) rank_emit<false>(A, rl, rg, nullptr, rec, j, -1);
      if (tid == 0) *head = RankHead{0, k, st, 0};
    }
    return;
  }
  int64_t lo = 0, hi = LIST ? (int64_t)A.parts * k : A.C;
  if (PART) {
    lo = (int64_t)part * A.slice;
    hi = lo + A.slice < A.C ? lo + A.slice : A.C;
  }
  const bool vec = !LIST && ((((uintptr_t)rl ^ (uintptr_t)rg) & 8) == 0);
  const int64_t p_first = lo - (vec ? (int64_t)(((uintptr_t)(rl + lo) >> 3) & 1) : 0);
  uint64_t key[2];
  int32_t idx[2];

  if constexpr (KMAX == 64) {
    __shared__ uint64_t s_k[NW][64];
    __shared__ int32_t s_i[NW][64];
    uint64_t bk = ~0ull;  // the wave's best list, one entry per lane
    int32_t bi = INT32_MAX;
    uint64_t tk = ~0ull;  // its k-th entry
    int32_t ti = INT32_MAX;
    for (int64_t p0 = p_first + (int64_t)wave * 128; p0 < hi; p0 += (int64_t)NW * 128) {  // (no barrier inside)
      rank_fetch2<LIST>(rl, rg, list, vec, p0 + 2 * lane, lo, hi, key, idx);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool in = key[e] <= RANK_KEY_PINF && topk_less(key[e], idx[e], tk, ti);
        if (__ballot(in)) {  // wave-uniform
          uint64_t ck = in ? key[e] : ~0ull;
          int32_t ci = in ? idx[e] : INT32_MAX;
          rank_wave_sort(ck, ci, lane);
          rank_wave_merge(bk, bi, ck, ci, lane);
          tk = (uint64_t)__shfl((unsigned long long)bk, k - 1);
          ti = __shfl(bi, k - 1);
        }
      }
    }
    if (NW > 1) {
      s_k[wave][lane] = bk;
      s_i[wave][lane] = bi;
      __syncthreads();
      if (wave != 0) return;
#pragma unroll
      for (int w = 1; w < NW; ++w) rank_wave_merge(bk, bi, s_k[w][lane], s_i[w][lane], lane);
    }
    const int nranked = (int)__popcll(__ballot(bk <= RANK_KEY_PINF));
    const int count = nranked < k ? nranked : k;
    if (lane < k) rank_emit<PART>(A, rl, rg, plist, rec, lane, lane < count ? bi : -1);
    if (!PART && lane == 0) *head = RankHead{count, k, st, 0};
  } else {
    __shared__ uint64_t sk[RANK_CAP];
    __shared__ int32_t si[RANK_CAP], sp[RANK_CAP];
    __shared__ int32_t swc[RANK_T / 64];
    __shared__ int32_t s_add[3];  // entrants of step c in s_add[c % 3]
    TopkRank<RANK_T> rank;
    rank.init(sk, si, sp, swc, RANK_CAP, k);
    if (tid < 3) s_add[tid] = 0;
    int c = 0;
    for (int64_t p0 = p_first; p0 < hi; p0 += 2 * RANK_T, ++c) {  // uniform trip count
      __syncthreads();                       // step c - 1 is staged and counted
      rank.pend += s_add[(c + 2) % 3];       // (step c - 1's counter: nobody adds to it any more)
      if (tid == 0) s_add[(c + 1) % 3] = 0;  // (step c - 2's: every thread read it before this step's barrier)
      if (rank.nb + rank.pend + 2 * RANK_T > RANK_CAP) rank.merge();  // uniform; afterwards nb <= k, pend = 0
      rank_fetch2<LIST>(rl, rg, list, vec, p0 + 2 * tid, lo, hi, key, idx);
      const bool in0 = key[0] <= RANK_KEY_PINF && rank.enters(key[0], idx[0]);
      const bool in1 = key[1] <= RANK_KEY_PINF && rank.enters(key[1], idx[1]);
      const uint64_t b0 = __ballot(in0), b1 = __ballot(in1);
      const int n0 = (int)__popcll(b0), n = n0 + (int)__popcll(b1);
      if (n) {  // wave-uniform
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_add[c % 3], n);
        base = __shfl(base, 0) + rank.nb + rank.pend;
        const uint64_t below = (1ull << lane) - 1ull;
        if (in0) {
          const int at = base + (int)__popcll(b0 & below);
          sk[at] = key[0];
          si[at] = idx[0];
          sp[at] = 0;
        }
        if (in1) {
          const int at = base + n0 + (int)__popcll(b1 & below);
          sk[at] = key[1];
          si[at] = idx[1];
          sp[at] = 0;
        }
      }
    }
    __syncthreads();
    if (c > 0) rank.pend += s_add[(c + 2) % 3];
    rank.finish();  // (ends with a barrier: [0, nb) is ranked, nb <= k)
    const int count = rank.nb;
    for (int j = tid; j < k; j += RANK_T) rank_emit<PART>(A, rl, rg, plist, rec, j, j < count ? si[j] : -1);
    if (!PART && tid == 0) *head = RankHead{count, k, st, 0};
  }
}

static int64_t rank_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the sizes every grid, index and list position relies on; the message names `who`
static int rank_check_sizes(const char* who, int64_t B, int64_t C, int32_t k) {
  if (B < 0 || C < 0) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld", who, (long long)B, (long long)C);
  if (k < 1 || k > HBX_RANK_MAX_K) return hbx_fail(HBX_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, HBX_RANK_MAX_K);
  if (k > C) return hbx_fail(HBX_ERR_ARG, "%s: k=%d exceeds C=%lld", who, k, (long long)C);
  if (B > INT32_MAX || (B > 0 && C > (int64_t)INT32_MAX / B))
    return hbx_fail(HBX_ERR_ARG, "%s: B * C = %lld * %lld exceeds int32", who, (long long)B, (long long)C);
  return HBX_OK;
}

static bool rank_sizes_ok(int64_t B, int64_t C, int32_t k) {
  return B >= 0 && k >= 1 && k <= HBX_RANK_MAX_K && k <= C && B <= INT32_MAX && !(B > 0 && C > (int64_t)INT32_MAX / B);
}

// the launches (every check is the callers')
static int rank_launch(RankArgs A, int64_t B, hipStream_t s) {
  const unsigned nb = (unsigned)B, np = (unsigned)(B * A.parts);  // B * parts <= B * C <= INT32_MAX
#define RANK_GO(KMAX, NW, LIST, PART, GRID) \
  hipLaunchKernelGGL((groups_rank_kernel<KMAX, NW, LIST, PART>), dim3(GRID), dim3(64 * NW), 0, s, A)
  if (A.parts > 1) {
    if (A.k <= 64) {
      RANK_GO(64, 4, false, true, np);
      HBX_LAUNCH_CHECK();
      if ((int64_t)A.parts * A.k <= 256)
        RANK_GO(64, 1, true, false, nb);
      else
        RANK_GO(64, 4, true, false, nb);
    } else {
      RANK_GO(HBX_RANK_MAX_K, 4, false, true, np);
      HBX_LAUNCH_CHECK();
      RANK_GO(HBX_RANK_MAX_K, 4, true, false, nb);
    }
  } else if (A.k > 64) {
    RANK_GO(HBX_RANK_MAX_K, 4, false, false, nb);
  } else if (A.C <= 256) {
    RANK_GO(64, 1, false, false, nb);
  } else {
    RANK_GO(64, 4, false, false, nb);
  }
#undef RANK_GO
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_rank_groups_workspace_bytes(int64_t B, int64_t C, int32_t k) {
  if (!rank_sizes_ok(B, C, k)) return -1;
  const int32_t parts = rank_parts(C);
  const int64_t lists = parts > 1 ? rank_align16(B * parts * (int64_t)k * (int64_t)sizeof(int32_t)) : 0;
  return lists > 16 ? lists : 16;  // (never 0: a caller can always allocate it)
}

int hbx_kde_rank_groups(const double* ln_l, const double* ln_g, const int32_t* status, int64_t B, int64_t C, int32_t k,
                        void* results, void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_rank_groups";
  if (const int rc = rank_check_sizes(who, B, C, k)) return rc;
  if (!ln_l || !ln_g || !status || !results || !workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if ((((uintptr_t)ln_l | (uintptr_t)ln_g | (uintptr_t)results) & 7) || ((uintptr_t)status & 3) ||
      ((uintptr_t)workspace & 15))
    return hbx_fail(HBX_ERR_ARG, "%s: pointers must be aligned (f64 and results: 8 bytes, i32: 4, workspace: 16)", who);
  const int64_t need = hbx_kde_rank_groups_workspace_bytes(B, C, k);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  if (B == 0) return HBX_OK;
  RankArgs A;
  A.ln_l = ln_l;
  A.ln_g = ln_g;
  A.status = status;
  A.C = C;
  A.k = k;
  A.parts = rank_parts(C);
  A.slice = (C + A.parts - 1) / A.parts;
  A.part = (int32_t*)workspace;
  A.out = (char*)results;
  return rank_launch(A, B, (hipStream_t)stream);
}

// the composite call's workspace: ln_l [B][C], ln_g [B][C], status [B], the ranking's lists, the ln-pdf's workspace
struct RankLayout {
  int64_t ln_g, status, rank, rank_bytes, logpdf, logpdf_bytes, total;
};
static bool rank_layout(int64_t B, int64_t C, int32_t k, int32_t D, RankLayout* L) {
  L->rank_bytes = hbx_kde_rank_groups_workspace_bytes(B, C, k);
  L->logpdf_bytes = hbx_kde_logpdf_groups_workspace_bytes(B, C, D);
  if (L->rank_bytes < 0 || L->logpdf_bytes < 0) return false;
  L->ln_g = rank_align16(B * C * (int64_t)sizeof(double));
  L->status = 2 * L->ln_g;
  L->rank = L->status + rank_align16(B * (int64_t)sizeof(int32_t));
  L->logpdf = L->rank + L->rank_bytes;
  L->total = L->logpdf + rank_align16(L->logpdf_bytes);
  return true;
}

int64_t hbx_kde_rank_logratio_groups_workspace_bytes(int64_t B, int64_t C, int32_t k, int32_t D) {
  RankLayout L;
  return rank_layout(B, C, k, D, &L) ? L.total : -1;
}

int hbx_kde_rank_logratio_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                 const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                 const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                 const int32_t* nlev_bad, const double* cand, int64_t C, int32_t k, double rtol,
                                 int32_t flags, void* results, void* workspace, int64_t ws_bytes, void* stream) {
  const char* who = "hbx_kde_rank_logratio_groups";
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (const int rc = rank_check_sizes(who, B, C, k)) return rc;
  if (!results || !workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if (((uintptr_t)results & 7) || ((uintptr_t)workspace & 15))
    return hbx_fail(HBX_ERR_ARG, "%s: results must be 8-byte, workspace 16-byte aligned", who);
  RankLayout L;
  if (!rank_layout(B, C, k, D, &L)) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld out of range", who, (long long)B, (long long)C);
  if (ws_bytes < L.total)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)L.total);
  if (B == 0) return HBX_OK;
  char* ws = (char*)workspace;
  double* ln_l = (double*)ws;
  double* ln_g = (double*)(ws + L.ln_g);
  int32_t* status = (int32_t*)(ws + L.status);
  // (the model pointers, cand, rtol and flags are checked there, before its first launch)
  if (const int rc = hbx_kde_logpdf_groups(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good,
                                           nlev_bad, cand, C, rtol, flags, ln_l, ln_g, status, ws + L.logpdf,
                                           L.logpdf_bytes, stream))
    return rc;
  return hbx_kde_rank_groups(ln_l, ln_g, status, B, C, k, results, ws + L.rank, L.rank_bytes, stream);
}

}  // extern "C"
