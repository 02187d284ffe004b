// hbx_impute.h -- the rules of conditional search spaces, host + device: imputation of a set's inactive (NaN)
// entries and deactivation of a row's inactive dims.  Users: hbx_impute.hip (the kernels and the host entries).
//
// Imputation.  A set is the ns rows j = 0 .. ns - 1 of a group's good or bad KDE in split order.  Per dim d the
// set carries a bitmask over j of the rows whose ORIGINAL value at d is not NaN (+-inf is a value), the number
// of set bits in the words before each word, and the total m_d.  Row j of the set, view row v, iteration
// t = 0, 1, ... while the row holds a NaN, with r = draw(seed, counter_base + v, IMPUTE_WORD0 + t, stream_id),
// u_a = hbx_u01_open(bits64(r, 0)), u_b = hbx_u01_open(bits64(r, 1)) and d0 the lowest NaN dim:
//   m_d0 > 0   donor = the k-th non-NaN row of d0 in ascending j, k = min(m - 1, floor(u_a m)); EVERY NaN dim of
//              the row takes the donor's original value, which may be NaN again (the loop goes on)
//   m_d0 == 0  dim d0 takes the prior: u_b where levels[d0] == 0, else min(L - 1, floor(L u_b)), L = levels[d0]
//              (hbx_groups_config.hip's prior rule)
// Every iteration fills d0, so the loop is bounded by D.  The only arithmetic is floor(u m) in fp64.
#pragma once
#include "hbx_common.h"
#include "hbx_philox.h"

static_assert(HBX_MAX_D == 256, "imp_row keeps a row's NaN dims in four 64-bit words");

#define IMP_NAN_BITS 0x7ff8000000000000ull  // the NaN a deactivated entry holds (numpy's np.nan)

// One set of one group.  mask / pre: [W][D] words (word w of dim d at w D + d), cnt: [D].
struct ImpSet {
  const double* Xs;     // the group's first original row
  const int64_t* ord;   // the set's ns positions local to the group, in split order
  int64_t ns;
  int32_t D, W;         // W = ceil(ns / 32)
  const uint32_t* mask; // bit j & 31 of word j >> 5: row j's original value at d is not NaN
  const uint32_t* pre;  // set bits of dim d in the words before w
  const uint32_t* cnt;  // m_d
  const int32_t* levels;
};

// position of the r-th (0-based) set bit of x; r < popcount(x)
__host__ __device__ __forceinline__ int imp_select32(uint32_t x, int r) {
  int pos = 0;
  for (int s = 16; s > 0; s >>= 1) {
    const int c = __builtin_popcount((x >> pos) & ((1u << s) - 1u));
    if (r >= c) {
      r -= c;
      pos += s;
    }
  }
  return pos;
}

// the set row that is the k-th (0-based, k < m_d) non-NaN row of dim d
__host__ __device__ __forceinline__ int64_t imp_kth_row(const ImpSet& S, int d, uint32_t k) {
  int lo = 0, hi = S.W - 1;  // the last word whose prefix count is <= k holds the bit
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S.pre[(int64_t)mid * S.D + d] <= k)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t at = (int64_t)lo * S.D + d;
  return (int64_t)lo * 32 + imp_select32(S.mask[at], (int)(k - S.pre[at]));
}

// Impute set row j in place: `out` holds the byte copy of the original row.  ctr: counter_base + view row.
// Adds the entries filled from donors / from the prior to *n_donor / *n_prior.
__host__ __device__ inline void imp_row(const ImpSet& S, int64_t j, double* out, uint64_t seed, uint64_t ctr,
                                        uint32_t stream_id, int32_t* n_donor, int32_t* n_prior) {
  const int D = S.D;
  const uint32_t* mrow = S.mask + (j >> 5) * (int64_t)D;
  const int sh = (int)(j & 31);
  uint64_t nan[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint64_t m = 0;
    for (int dd = 0; dd < 64 && q * 64 + dd < D; ++dd)
      if (!((mrow[q * 64 + dd] >> sh) & 1u)) m |= 1ull << dd;
    nan[q] = m;
  }
  int32_t nd = 0, np = 0;
  for (int t = 0; t < D; ++t) {
    int d0 = -1;
#pragma unroll
    for (int q = 3; q >= 0; --q)
      if (nan[q]) d0 = q * 64 + __builtin_ctzll(nan[q]);
    if (d0 < 0) break;
    const HbxU32x4 r = draw(seed, ctr, IMPUTE_WORD0 + (uint32_t)t, stream_id);
    const uint32_t m = S.cnt[d0];
    if (m > 0) {
      const double ua = hbx_u01_open(hbx_bits64(r, 0));
      uint32_t k = (uint32_t)(ua * (double)m);  // ua > 0: the truncation is the floor
      if (k > m - 1) k = m - 1;
      const double* drow = S.Xs + S.ord[imp_kth_row(S, d0, k)] * (int64_t)D;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint64_t bits = nan[q], keep = 0;
        while (bits) {
          const int dd = __builtin_ctzll(bits);
          bits &= bits - 1;
          const double v = drow[q * 64 + dd];
          out[q * 64 + dd] = v;
          if (v != v)
            keep |= 1ull << dd;
          else
            ++nd;
        }
        nan[q] = keep;
      }
    } else {
      const double ub = hbx_u01_open(hbx_bits64(r, 1));
      const int L = S.levels[d0];
      double v = ub;
      if (L > 0) {
        const int lv = (int)((double)L * ub);  // ub > 0: the truncation is the floor
        v = (double)(lv < L - 1 ? lv : L - 1);
      }
      out[d0] = v;
      ++np;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == (d0 >> 6)) nan[q] &= ~(1ull << (d0 & 63));
    }
  }
  *n_donor += nd;
  *n_prior += np;
}

// Deactivation.  Conditions i = 0 .. n_cond - 1 in topological order (a dim's own conditions before those it is
// the parent of): child[i] becomes NaN when the row's entry at parent[i] is NaN or is not an integer level in
// [0, 64) whose bit is set in allowed[i].  A condition that names a dim outside [0, D) is skipped.
__host__ __device__ inline void imp_deactivate_row(double* row, int32_t D, const int32_t* child,
                                                   const int32_t* parent, const uint64_t* allowed, int64_t n_cond) {
  for (int64_t i = 0; i < n_cond; ++i) {
    const int32_t c = child[i], p = parent[i];
    if (c < 0 || c >= D || p < 0 || p >= D) continue;
    const double v = row[p];
    bool on = false;
    if (v >= 0.0 && v < 64.0) {  // (false for NaN)
      const int lv = (int)v;
      on = (double)lv == v && ((allowed[i] >> lv) & 1ull);
    }
    if (!on) {
      const uint64_t nb = IMP_NAN_BITS;
      double nanv;
      __builtin_memcpy(&nanv, &nb, 8);
      row[c] = nanv;
    }
  }
}
