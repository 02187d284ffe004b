// hbx_groups_sh.hip -- grouped successive halving: every bracket's next stage from its promotion mask, on the device.
//
// hbx_sh_promote_ex leaves a mask per bracket; the next stage of bracket b is (HB_iteration.py:184-188, :135-138) the
// rows of its set positions in ascending position, then freshly sampled rows where crashed runs left slots empty.
// hbx_sh_advance_groups turns B masks into the stage tensor rows_out[B][K][D] and the map src_out[B][K]:
//
//   slot j <  min(a_b, K)            rows[seg_off[b] + p_j], p_j the j-th set position         src = p_j
//   the next f_b = min(F, K - ...)   fresh[b][i]                                              src = -1 - i
//   the rest                         the quiet NaN 0x7FF8000000000000 in every element        src = INT32_MIN
//
// Every row moves as 64-bit words (or pairs of them): no value is ever interpreted.
//
// Two steps, both by workgroups of SH_THREADS:
//   rank         the mask is walked in tiles of SH_TILE positions, SH_THREADS at a time: a wave ballots its 64 bytes,
//                the popcounts of the tile's 16 ballots go through LDS, and a set byte's rank is the count before the
//                tile + the popcounts of the ballots before its own + the set lanes below it (mbcnt).  Rank r < K
//                writes src_out[b][r]; the fill and NaN codes follow once a_b is known.
//   materialise  slot by slot from src_out: consecutive lanes take consecutive 16-byte pieces of a row (a row of
//                D = 32 is 16 lanes of 16 bytes), four pieces in flight per lane.  16-byte pieces only when D is even
//                and rows, fresh and rows_out are 16-byte aligned -- checked in the kernel --, else 8-byte ones.
//
// A bracket of at most SH_S1 positions does both in ONE workgroup of ONE launch (sh_advance_kernel): rank, a workgroup
// barrier, materialise from the src_out entries the workgroup has just written.  Longer brackets are cut into P equal
// slices (a multiple of SH_SUB positions each) and take three more launches on the same stream:
//   sh_count_kernel   block (p, b) counts slice p's set bytes into a scratch word,
//   sh_rank_kernel    block (p, b) sums the scratch words of the slices before its own (and all of them: a_b), ranks
//                     its slice and writes src_out; block (0, b) adds the fill / NaN codes and counts_out,
//   sh_gather_kernel  materialises the bracket's K slots, SH_GROWS slots per block.
// The stream orders the launches: no block ever waits for another one.  The scratch words are the first P int32 of the
// bracket's own rows_out[b] (2 K D int32 are there), which nothing reads or writes between the count and the gather
// that overwrites them, so the call needs no workspace and writes nothing outside its outputs.  The host knows B, K and
// D but no bracket length (seg_off stays on the device): P = min(SH_PMAX, SH_BLOCKS / B, 2 K D) is the same for every
// bracket, blocks of brackets that do not take their launch return at once, and with P < 2 (B > SH_BLOCKS / 2: the
// brackets themselves fill the machine) the three launches are not made and sh_advance_kernel takes every length.
#include "hbx_common.h"

#define SH_THREADS 256                 // one workgroup: 4 waves
#define SH_SUB SH_THREADS              // positions ranked per step of a tile (one ballot per wave)
#define SH_STEPS 4                     // steps per tile
#define SH_TILE (SH_SUB * SH_STEPS)    // 1024 positions between two exchanges of popcounts
#define SH_S1 8192                     // longest bracket of the one-workgroup route (when P >= 2)
#define SH_PMAX 256                    // slices of a long bracket at most (<= SH_THREADS: one scratch word per thread)
#define SH_BLOCKS 2048                 // blocks of a count / rank launch at most
#define SH_GROWS 64                    // slots per block of the gather launch
#define SH_GMAX 256                    // blocks per bracket of the gather launch at most
#define SH_NAN 0x7FF8000000000000ull
#define SH_NONE INT32_MIN

struct alignas(16) ShVec16 { uint64_t a, b; };
__device__ __forceinline__ void sh_nan(uint64_t& v) { v = SH_NAN; }
__device__ __forceinline__ void sh_nan(ShVec16& v) { v.a = SH_NAN; v.b = SH_NAN; }

__device__ __forceinline__ int sh_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// sum of `v` over the workgroup, in every thread; red: 4 words of LDS (reusable after the call's second barrier)
__device__ __forceinline__ uint32_t sh_block_sum(uint32_t v, uint32_t* red) {
  const uint32_t w = wave_reduce_dpp(v, OpAdd());
  __syncthreads();  // (the previous use of red is over)
  if ((threadIdx.x & 63) == 0) red[sh_wave()] = w;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Ranks the set bytes of positions [lo, hi) of one bracket's mask `adv`; `base` set bytes precede lo.  Rank r < K writes
// src[r] = position.  Returns the number of set bytes in [lo, hi) (the same in every thread).  cnt: SH_STEPS * 4 words.
__device__ __forceinline__ int64_t sh_rank_span(const uint8_t* __restrict__ adv, int64_t lo, int64_t hi, int64_t base,
                                                int64_t K, int32_t* src, uint32_t* cnt) {
  const int lane = threadIdx.x & 63, wave = sh_wave();
  const int64_t base0 = base;
  for (int64_t t0 = lo; t0 < hi; t0 += SH_TILE) {  // (uniform trip count)
    uint64_t bal[SH_STEPS];
#pragma unroll
    for (int r = 0; r < SH_STEPS; ++r) {
      const int64_t pos = t0 + r * SH_SUB + (int64_t)threadIdx.x;
      bal[r] = __ballot(pos < hi && adv[pos] != 0);
      if (lane == 0) cnt[r * 4 + wave] = (uint32_t)__popcll(bal[r]);
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (int r = 0; r < SH_STEPS; ++r) {
      uint32_t before = run;  // ballots of earlier steps, then the earlier waves of this step
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint32_t c = cnt[r * 4 + w];
        before += w < wave ? c : 0u;
        run += c;
      }
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[r] >> 32),
                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)bal[r], 0u));
      const int64_t rank = base + before + below;
      if (((bal[r] >> lane) & 1ull) && rank < K) src[rank] = (int32_t)(t0 + r * SH_SUB + (int64_t)threadIdx.x);
    }
    base += run;
    __syncthreads();  // (cnt is rewritten by the next tile)
  }
  return base - base0;
}

// the codes behind the advanced rows: fresh row i = -1 - i for the next f slots, SH_NONE for the rest
__device__ __forceinline__ void sh_fill_codes(int32_t* src, int64_t na, int64_t f, int64_t K) {
  for (int64_t j = na + threadIdx.x; j < K; j += SH_THREADS) src[j] = j - na < f ? (int32_t)(-1 - (j - na)) : SH_NONE;
}

// slots [j0, j1) of one bracket from their src codes; U pieces of type V per row
template <typename V>
__device__ __forceinline__ void sh_materialise(const V* __restrict__ rows, const V* __restrict__ fresh,
                                               V* __restrict__ out, const int32_t* src, int U, int64_t j0,
                                               int64_t j1) {
  const int dj = SH_THREADS / U, dc = SH_THREADS % U;  // one step of the workgroup, in (slot, piece)
  int64_t j = j0 + (int)threadIdx.x / U;
  int c = (int)threadIdx.x % U;
  while (j < j1) {
    int64_t jj[4];
    int cc[4], s[4];
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      jj[u] = j;
      cc[u] = c;
      c += dc;
      j += dj;
      if (c >= U) {
        c -= U;
        ++j;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = jj[u] < j1 ? src[jj[u]] : SH_NONE;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      sh_nan(v[u]);
      if (s[u] >= 0)
        v[u] = rows[(int64_t)s[u] * U + cc[u]];
      else if (s[u] != SH_NONE)
        v[u] = fresh[(int64_t)(-1 - s[u]) * U + cc[u]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (jj[u] < j1) out[jj[u] * U + cc[u]] = v[u];
  }
}

// 16-byte pieces where D and the three bases allow them (the bracket's offsets are then multiples of 16 bytes too)
__device__ __forceinline__ void sh_materialise_any(const double* rows_b, const double* fresh_b, double* out_b,
                                                   const int32_t* src_b, int32_t D, bool wide, int64_t j0, int64_t j1) {
  if (wide)
    sh_materialise<ShVec16>((const ShVec16*)rows_b, (const ShVec16*)fresh_b, (ShVec16*)out_b, src_b, D >> 1, j0, j1);
  else
    sh_materialise<uint64_t>((const uint64_t*)rows_b, (const uint64_t*)fresh_b, (uint64_t*)out_b, src_b, D, j0, j1);
}

__device__ __forceinline__ bool sh_wide(const double* rows, const double* fresh, const double* rows_out, int32_t D) {
  return !(D & 1) && !(((uintptr_t)rows | (uintptr_t)fresh | (uintptr_t)rows_out) & 15);
}

// one bracket: its length, its part of every array
struct ShBracket {
  int64_t n;
  const uint8_t* adv;
  const double *rows, *fresh;
  double* out;
  int32_t* src;
};
__device__ __forceinline__ ShBracket sh_bracket(int64_t b, const double* rows, int32_t D, const int64_t* seg_off,
                                                const uint8_t* advance, const double* fresh, int64_t F, int64_t K,
                                                double* rows_out, int32_t* src_out) {
  ShBracket g;
  const int64_t s = seg_off[b], e = seg_off[b + 1];
  g.n = e > s ? e - s : 0;
  g.adv = advance + s;
  g.rows = rows + s * (int64_t)D;
  g.fresh = fresh ? fresh + b * F * (int64_t)D : nullptr;
  g.out = rows_out + b * K * (int64_t)D;
  g.src = src_out + b * K;
  return g;
}

// the one-workgroup route: block b is bracket b (any length with long_route == 0, else up to SH_S1)
__global__ __launch_bounds__(SH_THREADS) void sh_advance_kernel(
    const double* __restrict__ rows, int32_t D, const int64_t* __restrict__ seg_off, const uint8_t* __restrict__ advance,
    const double* __restrict__ fresh, int64_t F, int64_t K, double* __restrict__ rows_out, int32_t* __restrict__ src_out,
    int64_t* __restrict__ counts_out, int long_route) {
  __shared__ uint32_t cnt[SH_STEPS * 4];
  const int64_t b = blockIdx.x;
  const ShBracket g = sh_bracket(b, rows, D, seg_off, advance, fresh, F, K, rows_out, src_out);
  if (long_route && g.n > SH_S1) return;  // (uniform)
  const int64_t a = sh_rank_span(g.adv, 0, g.n, 0, K, g.src, cnt);
  const int64_t na = a < K ? a : K;
  const int64_t f = g.fresh ? (F < K - na ? F : K - na) : 0;
  sh_fill_codes(g.src, na, f, K);
  if (counts_out && threadIdx.x == 0) {
    counts_out[2 * b] = a;
    counts_out[2 * b + 1] = f;
  }
  __syncthreads();  // the workgroup's src_out entries are read back below
  sh_materialise_any(g.rows, g.fresh, g.out, g.src, D, sh_wide(rows, fresh, rows_out, D), 0, K);
}

// slice p of a long bracket: positions [lo, hi)
__device__ __forceinline__ void sh_slice(int64_t n, int P, int p, int64_t& lo, int64_t& hi) {
  const int64_t L = ((n + P - 1) / P + SH_SUB - 1) / SH_SUB * SH_SUB;
  lo = p * L < n ? p * L : n;
  hi = lo + L < n ? lo + L : n;
}

__global__ __launch_bounds__(SH_THREADS) void sh_count_kernel(const int64_t* __restrict__ seg_off,
                                                              const uint8_t* __restrict__ advance, int32_t D, int64_t K,
                                                              double* __restrict__ rows_out) {
  __shared__ uint32_t red[4];
  const int64_t b = blockIdx.y;
  const int64_t s = seg_off[b], n = seg_off[b + 1] - s;
  if (n <= SH_S1) return;  // (uniform)
  int64_t lo, hi;
  sh_slice(n, (int)gridDim.x, (int)blockIdx.x, lo, hi);
  const uint8_t* adv = advance + s;
  uint32_t c = 0;
  for (int64_t pos = lo + threadIdx.x; pos < hi; pos += SH_THREADS) c += adv[pos] != 0;
  c = sh_block_sum(c, red);
  if (threadIdx.x == 0) ((uint32_t*)(rows_out + b * K * (int64_t)D))[blockIdx.x] = c;
}

__global__ __launch_bounds__(SH_THREADS) void sh_rank_kernel(const int64_t* __restrict__ seg_off,
                                                             const uint8_t* __restrict__ advance, int32_t D,
                                                             int has_fresh, int64_t F, int64_t K,
                                                             const double* __restrict__ rows_out,
                                                             int32_t* __restrict__ src_out,
                                                             int64_t* __restrict__ counts_out) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t cnt[SH_STEPS * 4];
  const int64_t b = blockIdx.y;
  const int64_t s = seg_off[b], n = seg_off[b + 1] - s;
  if (n <= SH_S1) return;  // (uniform)
  const int P = (int)gridDim.x, p = (int)blockIdx.x;
  const uint32_t* scratch = (const uint32_t*)(rows_out + b * K * (int64_t)D);
  const uint32_t mine = (int)threadIdx.x < P ? scratch[threadIdx.x] : 0u;
  const int64_t before = sh_block_sum((int)threadIdx.x < p ? mine : 0u, red);
  int64_t lo, hi;
  sh_slice(n, P, p, lo, hi);
  int32_t* src = src_out + b * K;
  sh_rank_span(advance + s, lo, hi, before, K, src, cnt);
  if (p == 0) {
    const int64_t a = sh_block_sum(mine, red);
    const int64_t na = a < K ? a : K;
    const int64_t f = has_fresh ? (F < K - na ? F : K - na) : 0;
    sh_fill_codes(src, na, f, K);
    if (counts_out && threadIdx.x == 0) {
      counts_out[2 * b] = a;
      counts_out[2 * b + 1] = f;
    }
  }
}

__global__ __launch_bounds__(SH_THREADS) void sh_gather_kernel(
    const double* __restrict__ rows, int32_t D, const int64_t* __restrict__ seg_off, const double* __restrict__ fresh,
    int64_t F, int64_t K, double* __restrict__ rows_out, const int32_t* __restrict__ src_out) {
  const int64_t b = blockIdx.y;
  const ShBracket g = sh_bracket(b, rows, D, seg_off, nullptr, fresh, F, K, rows_out, (int32_t*)src_out);
  if (g.n <= SH_S1) return;  // (uniform)
  const bool wide = sh_wide(rows, fresh, rows_out, D);
  for (int64_t j0 = (int64_t)blockIdx.x * SH_GROWS; j0 < K; j0 += (int64_t)gridDim.x * SH_GROWS)
    sh_materialise_any(g.rows, g.fresh, g.out, g.src, D, wide, j0, j0 + SH_GROWS < K ? j0 + SH_GROWS : K);
}

extern "C" {

int hbx_sh_advance_groups(const double* rows, int32_t D, const int64_t* seg_off, int64_t B, const uint8_t* advance,
                          const double* fresh, int64_t F, int64_t K, double* rows_out, int32_t* src_out,
                          int64_t* counts_out, void* stream) {
  const char* who = "hbx_sh_advance_groups";
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || K < 0 || F < 0)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld K=%lld F=%lld", who, (long long)B, (long long)K, (long long)F);
  if (B > INT32_MAX || K > INT32_MAX || F > INT32_MAX)  // (the grid; src_out's int32 codes)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld K=%lld F=%lld beyond int32", who, (long long)B, (long long)K, (long long)F);
  if (F > 0 && !fresh) return hbx_fail(HBX_ERR_ARG, "%s: F=%lld without fresh rows", who, (long long)F);
  if (B == 0 || K == 0) return HBX_OK;  // (no output has an element: the pointers are not looked at)
  if (!rows || !seg_off || !advance || !rows_out || !src_out) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if ((((uintptr_t)rows | (uintptr_t)fresh | (uintptr_t)rows_out | (uintptr_t)seg_off | (uintptr_t)counts_out) & 7) ||
      ((uintptr_t)src_out & 3))
    return hbx_fail(HBX_ERR_ARG, "%s: f64 / i64 pointers must be 8-byte, src_out 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  int64_t P = SH_BLOCKS / B;
  if (P > SH_PMAX) P = SH_PMAX;
  if (P > 2 * K * (int64_t)D) P = 2 * K * (int64_t)D;  // the scratch words live in the bracket's rows_out[b]
  const int long_route = P >= 2;
  hipLaunchKernelGGL(sh_advance_kernel, dim3((unsigned)B), dim3(SH_THREADS), 0, s, rows, D, seg_off, advance, fresh, F,
                     K, rows_out, src_out, counts_out, long_route);
  HBX_LAUNCH_CHECK();
  if (long_route) {  // (B <= SH_BLOCKS / 2: within the grid's y range)
    int64_t G = (K + SH_GROWS - 1) / SH_GROWS;
    if (G > SH_GMAX) G = SH_GMAX;
    hipLaunchKernelGGL(sh_count_kernel, dim3((unsigned)P, (unsigned)B), dim3(SH_THREADS), 0, s, seg_off, advance, D, K,
                       rows_out);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sh_rank_kernel, dim3((unsigned)P, (unsigned)B), dim3(SH_THREADS), 0, s, seg_off, advance, D,
                       fresh ? 1 : 0, F, K, rows_out, src_out, counts_out);
    HBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sh_gather_kernel, dim3((unsigned)G, (unsigned)B), dim3(SH_THREADS), 0, s, rows, D, seg_off, fresh,
                       F, K, rows_out, src_out);
    HBX_LAUNCH_CHECK();
  }
  return HBX_OK;
}

}  // extern "C"
