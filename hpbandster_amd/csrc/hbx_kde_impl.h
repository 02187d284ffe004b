// hbx_kde_impl.h -- definitions shared by the KDE scoring translation units (device code +
// chunk-layout helpers).  Split across files only so the template buckets compile in parallel.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hbx_common.h"

#define HBX_LN2f 0.69314718055994531f
#define HBX_LN_CLAMP (-18.420680743952367)   // ln(1e-8), bohb.py:129
// The score floor f of max(f, g) / max(l, f) (hbx_rules.pdf_floor; the reference snapshot's 1e-8) as the
// selection kernels take it: a launch argument, so kernel scalars, never a load.
//   C   (float)ln f.  For the default it is (float)HBX_LN_CLAMP bit for bit (the default is taken by value, not
//       through log(), so the default path cannot depend on the host's libm).
//   C1  C - margin: a ln-pdf upper bound below it is certainly under the floor.  The margin covers the rounding of
//       ln f to float (half an ulp of C) and log()'s own error: max(1e-4, 2 ulp_f32(C)) -- 1e-4 at the default and
//       over the whole accepted range (2 ulp = 3.1e-5 at |C| = 230, f = 1e-100), two ulps should the range ever grow.
//   w   what a score interval's ends are widened by where only one factor is clamped (both clamped: the score is
//       f / f = 1 exactly): the distance of C from ln f, one ulp of C.  0 for the default, whose 1e-6 the ln-pdf
//       intervals' own slack (1e-5 + 1e-6 |ln pdf|, est_interval) has always covered -- its intervals keep their bits.
struct ScoreFloor {
  double f;
  float C, C1, w;
};
#define HBX_PDF_FLOOR_DEFAULT 1e-8
#define HBX_PDF_FLOOR_MIN 1e-100
static inline bool hbx_pdf_floor_ok(double f) { return f >= HBX_PDF_FLOOR_MIN && f <= 1.0; }  // NaN, inf: false
static inline ScoreFloor hbx_score_floor(double f) {
  ScoreFloor r;
  r.f = f;
  r.C = f == HBX_PDF_FLOOR_DEFAULT ? (float)HBX_LN_CLAMP : (float)log(f);
  const float ulp = nextafterf(fabsf(r.C), INFINITY) - fabsf(r.C);
  const float margin = 2.f * ulp > 1e-4f ? 2.f * ulp : 1e-4f;
  r.C1 = r.C - margin;
  r.w = f == HBX_PDF_FLOOR_DEFAULT ? 0.f : ulp;
  return r;
}
// An entry point's hbx_rules (NULL: the reference snapshot's): HBX_ERR_ARG outside the accepted ranges
static inline int hbx_rules_check(const char* who, const hbx_rules* r) {
  if (!r) return HBX_OK;
  if (!hbx_pdf_floor_ok(r->pdf_floor))
    return hbx_fail(HBX_ERR_ARG, "%s: pdf_floor=%g outside [1e-100, 1]", who, r->pdf_floor);
  if (!(r->min_bandwidth >= 0.0) || isinf(r->min_bandwidth))
    return hbx_fail(HBX_ERR_ARG, "%s: min_bandwidth=%g is not finite and >= 0", who, r->min_bandwidth);
  return HBX_OK;
}
#define HBX_INV_SQRT_2PI 0.3989422804014327  // 1. / np.sqrt(2 * np.pi), SM:kernels.py:125
#ifndef EXACT_GRID
#define EXACT_GRID 2048  // blocks of the exact re-score (grid-stride over its work items)
#endif
#define SUM_BLOCK 32
#define OBS_CHUNK 64   // observations per table chunk (= per LDS stage of the scoring kernel)
#define KROW 80        // floats per k-row of a chunk: 64 observations + 16 pad (LDS bank spread)
#define MFMA_WAVES 8   // waves per scoring block; each wave owns 16 candidates
#ifndef H_ROW_TILES
#define H_ROW_TILES 2  // hmode: 16-candidate row tiles per wave (32 candidates)
#endif
// hmode: minimum waves per SIMD the register allocation must allow (128 VGPRs at 4)
#ifndef H_WAVES_PER_EU
#if H_ROW_TILES <= 2
#define H_WAVES_PER_EU 4
#else
#define H_WAVES_PER_EU 2
#endif
#endif
// hmode (16x16 tiles): waves per block, two blocks per CU.  (A 16-wave block with a 6-deep ring --
// half the LDS-DMA instructions per pair -- ended in a GPU memory fault on its first launch; cause not
// found, so it is not offered.)
#define H16_WAVES 8
// the coarse pre-screen instance of the 32x32 kernel: waves per block and minimum waves per SIMD
#ifndef H32C_WAVES
#define H32C_WAVES 8
#endif
#ifndef H32C_EU
#define H32C_EU 4
#endif
// ... and its candidate column tiles per wave: 2 = 64 candidates per wave, each A fragment read from LDS
// feeding both tiles' matrix instructions (half the LDS reads per pair)
#ifndef H32C_CT
#define H32C_CT 2  // phases in snake order (hbx_score_h32.hip chunk2s); 1 / 3 / 4 measured no faster
#endif
// ... and the widest candidate row (doubles, odd stride) it stages through LDS one column tile at a time: the
// block's LDS object holds 32 such rows per wave, 68 672 bytes with the parameters at 8 waves -- two blocks per CU
#define H32C_ROW_DS 33
// ... and the narrowest: from one 128-byte cache line per row on.  Below it two lanes' rows share a line, a load
// of the direct path touches 16 lines at most, and the copy through LDS only adds latency (measured at D = 8:
// config #2's scoring launch 22.2 us direct, 23.3 us staged; at D = 16: 31.7 against 27.1 us)
#define H32C_ROW_DMIN 16

// Observation table, chunked for the MFMA scoring kernel.  Chunk c holds observations 64c..64c+63:
//   [KP k-rows][KROW]   B operand, k-major: k=0 -> C_j, k=1 -> 1, k=2+c -> X'_jc, rest 0
//   [64][du_pad]        categorical codes (float), observation-major
// KP = dc_pad + 2 rounded up to a multiple of 4 (MFMA 16x16x4 K step).  Observations past n in the
// last chunk are padding with C_j = -1e30 (their terms are exactly 0).
//
// Categorical part when kc >= 1 (one-hot mode): 64 observations x kc*32 f16, observation-major,
// slot k = 2*t + p of one-hot position t = (dim u, level) holds delta_u's f16 hi (p=0) / lo (p=1)
// part when the observation has that level, else 0; for signed KDEs a second block of the same
// shape holds 1 in the hi slot of matches in dims with negative match weight (parity count).
#define OH_MAX_KC 4  // one-hot mode up to 4 f16 MFMA K-steps: sum over dims of levels <= 64
__host__ __device__ constexpr int kp_of(int dc_pad) { return (dc_pad + 2 + 3) & ~3; }
__host__ __device__ constexpr int cat_floats(int du_pad, int kc, int sgn) {
  return kc == 0 ? OBS_CHUNK * du_pad : OBS_CHUNK * kc * 16 * (sgn ? 2 : 1);
}
__host__ __device__ constexpr int chunk_floats(int dc_pad, int du_pad, int kc = 0, int sgn = 0) {
  return kp_of(dc_pad) * KROW + cat_floats(du_pad, kc, sgn);
}
// hmode (all-f16) chunk: [64 f32: C_j] [64 obs x KTP halves: hi/lo continuous + one-hot] [signed:
// 64 obs x KPP halves parity]; continuous slot k = 4c + pt of dim c holds (pt even ? Xh_c : Xl_c) so
// the four products xh.Xh + xh.Xl + xl.Xh + xl.Xl reassemble x''.X' (A side: pt < 2 ? xh : xl) --
// except for dims c = 0, 1, 2, whose lo.lo slot 4c+3 carries one of the three exact f16 pieces of
// C_j against A = 1 (the dropped lo.lo products, <= 2^-22 |x''_c||X'_c| each, are in the bound), so
// C_j enters the product on the matrix cores; c_i enters as the accumulator input.  Needs
// |C_j| <= H_CMAX (f16 range) and dc >= 3: hbx_kde_prepare falls back to the f32-MFMA kernels
// otherwise.  Rows are padded by 16 halves (32 B) so the 16 rows a wave reads spread over banks.
#define H_CMAX 60000.f  // |C_j| limit of the three-piece f16 split
__host__ __device__ constexpr int nsc_of(int dc_pad) { return (4 * dc_pad + 31) / 32; }
// row strides are 8*odd dwords: the 16 rows a ds_read_b128 lane group touches then cover all 64
// banks exactly once (conflict-free)
__host__ __device__ constexpr int h_ktp(int dc_pad, int kc) { return 32 * (nsc_of(dc_pad) + kc) + 16; }
__host__ __device__ constexpr int h_kpp(int kc) { return 32 * kc + 16; }
// padded to a multiple of 8 KB: every wave of the scoring block moves the same number of 1-KB
// LDS-DMA pieces per chunk (the counted vmcnt of the pipeline depends on it)
__host__ __device__ constexpr int h_chunk_floats(int dc_pad, int kc, int sgn) {
  return (OBS_CHUNK + OBS_CHUNK * h_ktp(dc_pad, kc) / 2 + (sgn ? OBS_CHUNK * h_kpp(kc) / 2 : 0) + 2047) & ~2047;
}
// h32 layout (hmode 2: 32x32 matrix tiles with the observations on the A side, hbx_score_h32.hip).
// Chunk = 64 observation rows of h32_ktp halves, no header:
//   [0, 16 nd)             dense, nd = h32_nd(nsc) K-steps of 16: slots 0-2 = the three f16 pieces of C_j
//                          (candidate side 1), slots 3-5 = 1 (candidate side: the three pieces of its
//                          shifted c_i), continuous dim c at slots 6 + 3c + {0,1,2} = (Xh, Xl, Xh) against
//                          the candidate's (xh, xh, xl): xh.Xh + xh.Xl + xl.Xh, the lo.lo product given up
//                          (<= 2^-22 |x''_c||X'_c|, in the bound); the rest 0
//   [16 nd, +16 kp)        one-hot hi part, 2:4-compressed (the sparse A operand of
//                          v_smfmac_f32_32x32x32_f16), kp = ceil(one-hot positions / 32) steps: step s,
//                          group g covers positions t0 = 32s + 4g .. t0 + 3 (dims start at even positions,
//                          so each aligned pair belongs to one dim and a group meets at most two dims);
//                          halves 16s + 2g, +1 = the f16 hi of delta_u for the observation's level in
//                          (t0, t0+1) and in (t0+2, t0+3), 0 where it has none
//   [16 nd + 16 kp, +16 kp) the lo parts of the same deltas, same places
//   [16 nd + 32 kp, ...)   sparse index words, shared by both parts: h32_ixw dwords; dword ksp h + s = the
//                          index nibbles (i0 in {0,1}, i1 in {2,3}) of groups 4h..4h+3 of step s -- for kp = 1
//                          at dword 2b + h with b = bit 4 of the row: the lanes read them as ds_read_b64
//                          (banks (a/4) mod 64 over 32-lane groups), and rows c, c + 16 of a tile, 16 x 4*odd
//                          dwords apart, would otherwise share banks
// The precise instance runs the hi and the lo steps (2 kp sparse instructions); the FAST one (the
// acquisition) only the hi steps, the lo part -- at most sum_u |delta_u - f16(delta_u)| in the exponent
// -- going into its bound.
// Row stride 4*odd dwords: the 16 rows (32 consecutive rows in two lane halves) a ds_read_b128 lane
// group reads then start on 16 distinct 4-bank groups -- conflict-free (MI355X_MICROARCH 'LDS': b128
// lane groups {0-3,12-15,20-27}, ...).  Chunks padded to 1 KB (LDS-DMA pieces).
//   [par, +16 kp)          signed KDEs only (par = the index words' end rounded to 8 halves): the parity
//                          product, 2:4-compressed like the one-hot part and sharing its index words:
//                          0.5 in the slot of the observation's level when its dim has a negative match
//                          factor, so the accumulated value is 0.5 x (matched negative dims)
// instances built: those whose registers fit 4 waves per SIMD (unsigned), 2 (signed) -- without spills,
// except the precise unsigned <4,1> (16 bytes; it only serves reported ln-pdfs, its FAST twin has none)
__host__ __device__ constexpr int h32_nd(int nsc) { return (6 + 24 * nsc + 15) / 16; }  // dense K-steps
__host__ __device__ constexpr int h32_kp(int kc) { return (kc + 1) / 2; }  // 32-position steps of kc 16-position ones
__host__ __device__ constexpr bool h32_ok(int nsc, int kp, int sgn = 0) {
  return kp <= 2 && (h32_nd(nsc) + 2 * kp <= 8 || (nsc == 4 && kp == 1)) && (!sgn || kp >= 1);
}
__host__ __device__ constexpr int h32_ksp(int kp) { return kp == 3 ? 4 : kp; }  // index dwords per lane half
__host__ __device__ constexpr int h32_ixw(int kp) { return kp == 1 ? 4 : 2 * h32_ksp(kp); }  // index dwords per row
__host__ __device__ constexpr int h32_par(int nsc, int kp) {  // parity block offset (halves, 16-byte aligned)
  return (16 * h32_nd(nsc) + 32 * kp + 2 * h32_ixw(kp) + 7) & ~7;
}
__host__ __device__ constexpr int h32_ktp(int nsc, int kp, int sgn = 0) {
  return 8 * (((h32_par(nsc, kp) + (sgn ? 16 * kp : 0) + 7) / 8) | 1);
}
__host__ __device__ constexpr int h32_chunk_floats(int nsc, int kp, int sgn = 0) {
  return (OBS_CHUNK * h32_ktp(nsc, kp, sgn) / 2 + 255) & ~255;
}
#define H32_ROW_MAX 112  // dense halves of the largest h32 row (nsc = 4: 7 steps)
// Coarse h32 layout (hbx_score_h32.hip <CO = true>: the acquisition's pre-screen instance, unsigned KDEs):
// ONE f16 product per continuous dim.  Row = [16 ndc dense: slots 0-2 the C_j pieces, 3-5 = 1, 6 + c = Xh
// of continuous dim c] [16 kp one-hot hi part, 2:4-compressed as above] [index words as above]; no lo
// parts.  xh.Xh stands for x''.X': the dropped xh.Xl + xl.X' (<= |xh| (2^-11 xmax + 2^-25) + |xl| xmax per
// dim, log2 units) goes into the candidate's bound, and the exact re-score resolves what it leaves near
// the minimum.  2 dense + 1 sparse matrix instructions per 1024 pairs at 24c + 8u instead of 6.  The
// table is a second region of the same buffer (KdeParams::coarse_off floats in).
__host__ __device__ constexpr int h32c_nd(int nsc) { return (6 + 8 * nsc + 15) / 16; }
__host__ __device__ constexpr int h32c_par(int nsc, int kp) { return (16 * h32c_nd(nsc) + 16 * kp + 2 * h32_ixw(kp) + 7) & ~7; }
__host__ __device__ constexpr int h32c_ktp(int nsc, int kp) { return 8 * (((h32c_par(nsc, kp) + 7) / 8) | 1); }
__host__ __device__ constexpr int h32c_chunk_floats(int nsc, int kp) {
  return (OBS_CHUNK * h32c_ktp(nsc, kp) / 2 + 255) & ~255;
}
// The variant code of a prepared KDE (hbx_kde_prepare's info[0]; the bit layout: include/hbx.h at
// hbx_kde_prepare), the one place that packs and unpacks it.  Flags are 0 / 1.
struct KdeVariant {
  int has_neg;      // signed sums
  int kc;           // one-hot K-steps (0: categorical match on the VALU)
  int hmode;        // whole exponent on the f16 matrix cores
  int exact_only;   // outside every fp32 scoring bucket
  int h32;          // the 32x32-tile kernels (h32 table)
  int coarse;       // the table carries the coarse h32 layout
  int small_codes;  // <= 8 categorical slots, codes in [0, 3] (hbx_logpdf.hip DD_LUT)
  __host__ __device__ int encode() const {
    return has_neg | (kc << 1) | (hmode << 4) | (exact_only << 5) | (h32 << 6) | (coarse << 7) | (small_codes << 8);
  }
  __host__ __device__ static KdeVariant decode(int v) {
    return {v & 1, (v >> 1) & 7, (v >> 4) & 1, (v >> 5) & 1, (v >> 6) & 1, (v >> 7) & 1, (v >> 8) & 1};
  }
};

// ------------------------------------------------------------------------------------------
// fp32 log-domain scoring
//
// Per (candidate i, observation j), in log2 units and minus the static bound M0:
//   t_ij = C_j + c_i + sum_c x''_ic X'_jc + sum_u delta_u [x_iu == X_ju]
// with X' = s (X - mu), x'' = 2 s (x - mu), c_i = -|x'_i|^2, C_j = -|X'_j|^2 + lb_sum - M0
// (the expansion of -|x' - X'|^2).  The first three terms are one GEMM-shaped product
// [candidates x K] . [K x observations] with K = 2 + Dc: they run on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain in k order).  The categorical match,
// exp2 and the sums run on the VALU beside them.  The categorical match is m = clamp(1 - d*d) on
// the integer codes (d = x - X), which stays in the VALU (no VCC round trip).

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float cat_match(float a, float b) {
  const float d = a - b;
  return __builtin_amdgcn_fmed3f(fmaf(-d, d, 1.f), 0.f, 1.f);
}

__device__ __forceinline__ float cand_code(double xv) {
  // codes are integers; anything else (incl. NaN) never equals an observed code
  return (xv == rint(xv) && fabs(xv) < 1e6) ? (float)xv : -1e9f;
}

// Per-candidate epilogue: ln S+, ln S-, error bound (or the rescue marker err = -1).  sum_terms bounds
// the relative rounding error of the fp32 sums in units of 2^-24 (sequential additions along the
// longest accumulation path).
__device__ __forceinline__ KdeEst finish_est_terms(const KdeParams* __restrict__ P, float S, float Sn, float off,
                                                   bool nan_c, float ci, float bnd, bool SIGNED, float sum_terms) {
  KdeEst o;
  o.pad = 0.f;
  if (nan_c || S != S) {
    o.lpos = NAN;
    o.lneg = -INFINITY;
    o.err = 0.f;
    return o;
  }
  const float lnorm = (float)P->log_norm;
  const float Sp = SIGNED ? (S - Sn) : S;
  o.lpos = (Sp > 0.f) ? (__log2f(Sp) + off) * HBX_LN2f + lnorm : -INFINITY;
  o.lneg = (SIGNED && Sn > 0.f) ? (__log2f(Sn) + off) * HBX_LN2f + lnorm : -INFINITY;
  const float u = 0x1p-24f;
  const float Mabs = fabsf(ci) + P->cmax + bnd + P->sum_abs_delta;
  const float dt = 3.f * (float)(P->dc + P->du + 4) * u * Mabs;  // |error of t|, log2 units
  const float es = sum_terms * u * (SIGNED ? 3.f : 1.f);
  o.err = 2.f * (dt * HBX_LN2f + es) + 16.f * u;
  return o;
}
// ... the same operations on copies of the four fields it reads, for a kernel that finishes every candidate behind
// a long loop and loads them once, ahead of it (the coarse 32x32 instances): lnorm = (float)log_norm, dims = dc + du
struct EstPrm {
  float lnorm, cmax, sum_abs_delta;
  int32_t dims;
};
__device__ __forceinline__ KdeEst finish_est_terms(const EstPrm q, float S, float Sn, float off, bool nan_c, float ci,
                                                   float bnd, bool SIGNED, float sum_terms) {
  KdeEst o;
  o.pad = 0.f;
  if (nan_c || S != S) {
    o.lpos = NAN;
    o.lneg = -INFINITY;
    o.err = 0.f;
    return o;
  }
  const float Sp = SIGNED ? (S - Sn) : S;
  o.lpos = (Sp > 0.f) ? (__log2f(Sp) + off) * HBX_LN2f + q.lnorm : -INFINITY;
  o.lneg = (SIGNED && Sn > 0.f) ? (__log2f(Sn) + off) * HBX_LN2f + q.lnorm : -INFINITY;
  const float u = 0x1p-24f;
  const float Mabs = fabsf(ci) + q.cmax + bnd + q.sum_abs_delta;
  const float dt = 3.f * (float)(q.dims + 4) * u * Mabs;  // |error of t|, log2 units
  const float es = sum_terms * u * (SIGNED ? 3.f : 1.f);
  o.err = 2.f * (dt * HBX_LN2f + es) + 16.f * u;
  return o;
}

__device__ __forceinline__ KdeEst finish_est(const KdeParams* __restrict__ P, float S, float Sn, float off,
                                             bool nan_c, float ci, float bnd, bool SIGNED, int chunk) {
  return finish_est_terms(P, S, Sn, off, nan_c, ci, bnd, SIGNED,
                          (float)chunk + (float)P->n / (float)chunk + 24.f);
}

// A wave copies its nv candidate rows (contiguous in HBM: nv * D doubles from src) into LDS rows of
// stride DS, 16 loads per lane in flight at a time (a per-row loop would wait one memory latency per
// row: ~16 serialized HBM round trips per wave at D = 32, the largest piece of a block's prologue).
__device__ __forceinline__ void stage_rows(const double* __restrict__ src, int64_t nv, int D, int DS, double* xs,
                                           int lane) {
  if (D <= 64) {  // rows of D <= 64: lane = (row in pass, column), one division per lane instead of one per element
    const int rpp = 64 / D;  // rows per pass (uniform)
    const int lr = lane / D, lc = lane - lr * D;
    if (lr < rpp) {
      // the whole passes: uniform bases, one per-lane offset, up to 16 loads in flight, no per-element index
      // arithmetic and only uniform guards; then the ragged last pass (rows past nv masked)
      const int npf = (int)nv / rpp;
      const unsigned vo = (unsigned)(lr * D + lc), xo = (unsigned)(lr * DS + lc);
      const int sq = __builtin_amdgcn_readfirstlane(rpp * D), xq = __builtin_amdgcn_readfirstlane(rpp * DS);
      for (int p0 = 0; p0 < npf; p0 += 16) {
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (p0 + q < npf) t[q] = (src + (int64_t)(p0 + q) * sq)[vo];
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (p0 + q < npf) (xs + (p0 + q) * xq)[xo] = t[q];
      }
      const int row = npf * rpp + lr;
      if (row < (int)nv) xs[row * DS + lc] = src[row * D + lc];
    }
    return;
  }
  const int tot = (int)nv * D;
  for (int e0 = 0; e0 < tot; e0 += 16 * 64) {
    double t[16];
    int at[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = min(e0 + 64 * q + lane, tot - 1);  // past the end: the last element again
      const int row = e / D;
      at[q] = row * DS + (e - row * D);
      t[q] = src[e];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) xs[at[q]] = t[q];
  }
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));

typedef void (*logpdf_fn)(const double*, int64_t, int32_t, const KdeParams*, const float*, KdeEst*);

// kernel arguments of the two-KDE (l and g in one grid) hmode launch
#ifndef HBX_PAIR_INIT
#define HBX_PAIR_INIT 1  // the 32x32 pair kernel initialises a single acquisition's state (0: A/B builds only)
#endif

struct KdePairArgs {
  const KdeParams* P0;
  const KdeParams* P1;
  const float* table0;
  const float* table1;
  KdeEst* out0;
  KdeEst* out1;
  unsigned nblk0;
  // acquisition workspace counter of rescue-marked candidates (nullable): the scoring kernel counts its
  // markers, the rescue pass (or the combine kernel doing it) exits at once on 0, the shortlist kernel
  // zeroes it for the next acquisition
  int32_t* rescue;
  // single acquisition (nullable): the per-acquisition state the 32x32 pair kernel or the rescue pass
  // initialises in its first block (acq_init's work, one launch less): U, count, flags, first1, the record
  struct AcqInitPtrs {
    uint32_t* U;
    int32_t* count;
    int32_t* flags;
    int32_t* first1;
    struct AcqResult* res;
  } init;
  // observation splits (h32 pair kernels, acquisitions only): KDE k's blocks are `tiles` candidate tiles x
  // nsplit_k chunk ranges; range r writes its partial estimate to out_k + r Nc (the combine kernel merges
  // them).  1: one block covers all of the KDE's observations.
  unsigned tiles = 0;
  int32_t nsplit0 = 1, nsplit1 = 1;
  // the coarse 32x32 instances stage their candidate rows through LDS (0: HBX_ROW_STAGE=0, every lane reads its
  // row from global memory; the other instances do not look at it)
  int32_t row_stage = 1;
  // stage 1 of the staged argmin, unsplit (hbx_staged.hip; both null otherwise): the coarse pair kernels' (two
  // tiles or one) epilogue also leaves candidate i's ln-pdf interval's upper end in lhi[i] (NaN: l is NaN; +inf: rescue-marked,
  // the seed kernel re-scores it) and, per block, the largest lower end over its unmarked candidates in
  // bmax[block] (-inf: none)
  float* lhi = nullptr;
  float* bmax = nullptr;
};
typedef void (*logpdf_pair_fn)(const double*, int64_t, int32_t, KdePairArgs);
// the coarse 32x32 instance over one KDE: logpdf_fn's arguments and KdePairArgs::row_stage
typedef void (*logpdf_co_fn)(const double*, int64_t, int32_t, const KdeParams*, const float*, KdeEst*, int32_t);

// kernel arguments of a list launch (hbx_score_h32.hip kde_logpdf_h32_list_kernel; the staged acquisition,
// hbx_staged.hip): the candidates idx[0 .. min(*count, maxcount)) against one KDE.  At most cap listed: tiles_cap
// tiles x nsplit observation ranges, range r's partial estimate of list entry k at part[r cap + k] (merged and
// scattered by staged_merge_kernel); more: one unsplit block per tile, entry k's estimate straight to out[idx[k]].
// The grid is sized on the host for the list's capacity; blocks past the count exit after one load.
struct KdeListArgs {
  const KdeParams* P;
  const float* table;
  KdeEst* out;
  KdeEst* part;
  const int32_t* idx;
  const int32_t* count;
  int32_t* rescue;  // marker count (KdePairArgs::rescue)
  int32_t cap, maxcount, nsplit;
  unsigned tiles_cap;
  int32_t row_stage;  // KdePairArgs::row_stage
};
typedef void (*logpdf_list_fn)(const double*, int32_t, KdeListArgs);

// the staged acquisition's state words (hbx_staged.hip), in the result slot's padding right behind the record
// (WsLayout::stage): whether the call staged, Lmax and U_seed as order-preserving uints, the seed and survivor
// counts, the length of the short tail's preliminary shortlist, whether stage 1's epilogue left lhi.  They stay in the
// workspace after the call
// (hbx_kde_acquire_stats).
enum {
  HBX_ST_FLAG = 0,
  HBX_ST_LMAX,
  HBX_ST_USEED,
  HBX_ST_NSEED,
  HBX_ST_NSURV,
  HBX_ST_NPRE,
  HBX_ST_LHI1,  // 1: the call's lhi and Lmax came from stage 1's epilogue (hbx_kde_acquire_stage1)
  HBX_ST_WORDS
};

// a single acquisition's state before its combine / shortlist / exact / final steps; res is the workspace's
// result slot (256 bytes: the state words of a staged call follow the record)
__device__ __forceinline__ void acq_init_state(uint32_t* U, int32_t* count, int32_t* flags, int32_t* first1,
                                               AcqResult* res) {
  uint32_t* st = (uint32_t*)(res + 1);
  st[HBX_ST_FLAG] = 0;
  st[HBX_ST_LMAX] = hbx_f2ord(-INFINITY);
  st[HBX_ST_USEED] = hbx_f2ord(INFINITY);
  st[HBX_ST_NSEED] = 0;
  st[HBX_ST_NSURV] = 0;
  st[HBX_ST_NPRE] = 0;
  st[HBX_ST_LHI1] = 0;
  *U = hbx_f2ord(INFINITY);
  *first1 = INT32_MAX;
  *count = 0;
  *flags = 0;
  res->index = -1;
  res->score = NAN;
  res->pdf_l = NAN;
  res->pdf_g = NAN;
  res->shortlist = 0;
  res->flags = 0;
  res->near = 0;
  res->rel = 0.f;
}

// A partial estimate over an empty chunk range (S = 0): merging it changes nothing
__host__ __device__ inline KdeEst kde_est_neutral() {
  KdeEst e;
  e.lpos = -INFINITY;
  e.lneg = -INFINITY;
  e.err = 0.f;
  e.pad = 0.f;
  return e;
}

// Chunk range [c0, c0 + nch) of observation split r of nsplit over nchunks chunks (nch <= 0: empty)
__host__ __device__ inline void obs_split_range(int nchunks, int r, int nsplit, int* c0, int* nch) {
  const int per = (nchunks + nsplit - 1) / nsplit;
  *c0 = r * per;
  const int e = (*c0 + per) < nchunks ? (*c0 + per) : nchunks;
  *nch = e - *c0;
}

// one-call refit (hbx_kde_refit): the split metadata hbx_seg_argsort / hbx_kde_fit read from device memory,
// written by a kernel from its arguments (no host copy)
struct RefitMeta {
  int64_t seg[2];
  int64_t n_good, n_bad;
  double fac_good, fac_bad;
  int32_t vt[HBX_MAX_D];
};
struct RefitMetaArgs {
  int64_t n, n_good, n_bad;
  double fac_good, fac_bad;
  int32_t D;
  uint32_t vt[HBX_MAX_D / 32];
};
// hbx_fit.hip: append the staged rows, write the metadata and sort a refit's n <= REFIT_SORT_SMALL losses in
// numpy's order -- one launch for what the metadata kernel, the counting rank and the tie check did in five
#define REFIT_SORT_SMALL 1024
#define REFIT_INLINE 256  // appended doubles (rows, then losses) carried in that launch's kernel arguments
// staged: device rows to append, or (staged_inline non-null) host rows copied into the kernel arguments
int refit_sort_small(double* X, double* loss, const double* staged, const double* staged_inline, int64_t n_new,
                     const RefitMetaArgs& a, RefitMeta* m, int64_t* order, int32_t* arrays, hipStream_t s);

int refit_fit_colstats(const double* X, int32_t D, const int64_t* seg_off, const int64_t* order, const int64_t* n_good,
                       const int64_t* n_bad, const double* fac_good, const double* fac_bad, const int32_t* vartype,
                       double* bw_good, double* bw_bad, int32_t* nlev_good, int32_t* nlev_bad, ColStats* cs_good,
                       ColStats* cs_bad, double min_bw, hipStream_t s);
#define FIT_TILE_ROWS 16384  // kde_fit_col_kernel's LDS tile (FIT_TILE)

// host-side pickers of the scoring kernel instances (null pointers when the bucket has none), each with the block
// its file's kernels are compiled for: candidates and threads per block, from the constants of their
// __launch_bounds__ and tile loops
struct ScoreInst {
  logpdf_fn main = nullptr;
  logpdf_pair_fn pair = nullptr;  // l + g in one launch (hbx_score_h.hip)
  int cands_per_block = 0, threads = 0;
};
ScoreInst hbx_pick_f32(int dc_pad, int du_pad, bool sg);  // hbx_score_f32.hip
ScoreInst hbx_pick_oh(int dc_pad, int kc, bool sg);       // hbx_score_oh.hip
ScoreInst hbx_pick_h(int nsc, int kc, bool sg);           // hbx_score_h.hip
// hbx_score_h32.hip.  coarse (unsigned sums only): pair is the coarse pair kernel, and with it come its twin with
// one column tile per wave (half the candidates per block), the coarse instance over an index list (staged
// acquisition) and over one KDE (launched in main's place); the block is theirs
struct H32Inst {
  logpdf_fn main = nullptr;
  logpdf_pair_fn pair = nullptr, pair1 = nullptr;
  logpdf_list_fn list = nullptr;
  logpdf_co_fn main_co = nullptr;
  int cands_per_block = 0, threads = 0;
};
H32Inst hbx_pick_h32(int nsc, int kp, bool sg, bool fast, bool coarse);

// what the ln-pdf contract (hbx_logpdf.hip, hbx_kde_logpdf_rtol) launches from other units: hbx_score.hip's
// precise estimate instance of a bucket (main + rescue into est; HBX_ERR_UNSUPPORTED when it has none) ...
int hbx_logpdf_estimate(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                        int32_t dc_pad, int32_t du_pad, int32_t variant, KdeEst* est, hipStream_t s);
// ... and hbx_exact.hip's fp64 evaluation of the listed candidates list[0 .. *count): per_point = the
// one-block-per-point log-space kernel (buckets without a tiled instance), then ln of the exact pdf (negative
// categorical factors, structural NaN; its blocks exit for other KDEs)
int hbx_logpdf_exact_listed(const double* cand, int64_t Nc, int32_t D, const KdeParams* P, const double* X,
                            const int64_t* rows, double* out, const int32_t* list, const int32_t* count,
                            bool per_point, hipStream_t s);
