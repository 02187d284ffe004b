// hbx_groups_config.hip -- grouped get_config: a valid configuration per request, on the device.
//
// The grouped acquisitions (hbx_groups.hip) answer a request with a record: the index of the best candidate of its
// pool, or -1.  The reference's get_config (bohb.py:104-169) always returns a configuration: it draws from the prior
// when the run has no model or np.random.rand() < random_fraction (bohb.py:107-111), when no candidate has a score
// below +inf (best_vector is None, bohb.py:154-157) and when the sampler raises (bohb.py:163-166).  The finish launch
// here applies that rule to B * S records and their pools and writes the B * S configuration vectors and a source
// code per request.  Request q = b S + s, first matching rule:
//
//   2 NO_MODEL         flags & (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED), or no records at all     prior draw
//   1 RANDOM_FRACTION  u_q < random_fraction                                                      prior draw
//   4 DOMAIN_ERR       a byte of domain_err[q][0..C) is not zero                                  prior draw
//   3 NO_SCORE         index < 0 (or not below C: never written by the acquisitions, never read)  prior draw
//   0 MODEL            otherwise                                              cands[q][index][:], bit for bit
//
// The request-level draws sit on the request's first candidate counter ctr_q = counter_base + q C -- the sampler's
// seed and stream -- under words the sampler never uses (hbx_philox.h): DECIDE_WORD gives u_q, PRIOR_WORD0 + p the
// prior of dims 2p (bits64(r, 0)) and 2p + 1 (bits64(r, 1)).  With u = hbx_u01_open(bits): a continuous dim
// (levels[d] == 0) is u (configspace.py:62), a categorical dim of t levels min(t - 1, floor(t u))
// (configspace.py:97,113).  A group's answers depend on its own counters only, so they do not change with the other
// groups of the call.
//
// One wave per request, FIN_WAVES requests per block, lane = dim (a request with D > 64 loops).  Everything that
// decides the source is the same in all lanes of the wave -- one record, one draw, a ballot over the error bytes --
// and goes through readfirstlane, so the branches are scalar ones.  Lanes 2p and 2p + 1 compute the same Philox
// block and take one half each.  No LDS.
//
// hbx_kde_propose_groups is the composition hbx_kde_sample_groups (pool S C) -> hbx_kde_acquire_groups_batch ->
// the finish launch on one stream; it calls the two existing entry points as they are.
//
// The request mask (hbx_kde_finish_groups_m, want: u8[B][S]) adds a rule ahead of the five: an unwanted request gets
//   5 SKIPPED          want[q] == 0                                                           NaN row
// and every wanted request goes by the table above -- the <MASK = false> instance is the kernel it has always been.
// hbx_kde_random_requests_groups writes want and not (u_q < random_fraction), the requests a model has to answer: rule 1
// comes before the rules that read the pool, so hbx_kde_propose_groups_m with HBX_PROPOSE_SKIP_RANDOM samples and
// scores under that mask, finishes under `want`, and returns the rows and sources of the call without the flag.
#include "hbx_common.h"
#include "hbx_groups_impl.h"  // grp_counts_ok
#include "hbx_philox.h"

#define FIN_WAVES 4  // requests per block

template <bool MASK>
__global__ __launch_bounds__(64 * FIN_WAVES) void groups_finish_kernel(
    const AcqResult* __restrict__ records, const double* __restrict__ cands, const uint8_t* __restrict__ domain_err,
    const int32_t* __restrict__ levels, int32_t D, int64_t Q, int64_t C, double random_fraction, uint64_t seed,
    uint64_t counter_base, uint32_t stream_id, double* __restrict__ rows_out, uint8_t* __restrict__ source_out,
    const uint8_t* __restrict__ want) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * FIN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (q >= Q) return;  // (wave-uniform; no barrier below)
  if constexpr (MASK) {
    if (__builtin_amdgcn_readfirstlane((int)want[q]) == 0) {  // one byte for the wave: a scalar branch
      for (int d = lane; d < D; d += 64) rows_out[q * (int64_t)D + d] = NAN;
      if (lane == 0) source_out[q] = (uint8_t)HBX_CFG_SKIPPED;
      return;
    }
  }
  const uint64_t ctr = counter_base + (uint64_t)(q * C);
  int src = HBX_CFG_NO_MODEL;
  int64_t index = -1;
  if (records) {
    const AcqResult rec = records[q];  // one address for the wave
    if (!(rec.flags & (HBX_ACQ_NO_MODEL | HBX_ACQ_UNSUPPORTED))) {
      const double uq = hbx_u01_open(hbx_bits64(draw(seed, ctr, DECIDE_WORD, stream_id), 0));
      index = rec.index;
      src = uq < random_fraction ? HBX_CFG_RANDOM_FRACTION : HBX_CFG_MODEL;
    }
  }
  src = __builtin_amdgcn_readfirstlane(src);
  if (src == HBX_CFG_MODEL) {
    bool err = false;
    if (domain_err) {
      const uint8_t* e = domain_err + q * C;
      for (int64_t c0 = 0; c0 < C; c0 += 64) {  // (uniform trip count)
        const int64_t c = c0 + lane;
        err |= __ballot(c < C && e[c] != 0) != 0ull;
      }
    }
    const bool scored = index >= 0 && index < C;
    src = __builtin_amdgcn_readfirstlane(err ? HBX_CFG_DOMAIN_ERR : scored ? HBX_CFG_MODEL : HBX_CFG_NO_SCORE);
  }
  double* out = rows_out + q * (int64_t)D;
  if (src == HBX_CFG_MODEL) {
    const double* row = cands + (q * C + index) * (int64_t)D;
    for (int d = lane; d < D; d += 64) out[d] = row[d];
  } else {
    for (int d = lane; d < D; d += 64) {
      const HbxU32x4 r = draw(seed, ctr, PRIOR_WORD0 + (uint32_t)(d >> 1), stream_id);
      // (a select of two constant halves: indexing r by d & 1 would put the block in LDS)
      const double u = hbx_u01_open((d & 1) ? hbx_bits64(r, 1) : hbx_bits64(r, 0));
      const int t = levels[d];
      double v = u;
      if (t > 0) {
        const int lv = (int)((double)t * u);  // u > 0: the truncation is the floor
        v = (double)(lv < t - 1 ? lv : t - 1);
      }
      out[d] = v;
    }
  }
  if (lane == 0) source_out[q] = (uint8_t)src;
}

// want_out[q] = (want_in == NULL or want_in[q] != 0) and not (u_q < random_fraction), u_q the finish step's own draw
__global__ __launch_bounds__(256) void groups_random_requests_kernel(int64_t Q, int64_t C, double random_fraction,
                                                                     uint64_t seed, uint64_t counter_base,
                                                                     uint32_t stream_id,
                                                                     const uint8_t* __restrict__ want_in,
                                                                     uint8_t* __restrict__ want_out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const uint64_t ctr = counter_base + (uint64_t)(q * C);
  const double uq = hbx_u01_open(hbx_bits64(draw(seed, ctr, DECIDE_WORD, stream_id), 0));
  want_out[q] = (uint8_t)((!want_in || want_in[q] != 0) && !(uq < random_fraction));
}

// the checks the finish step and the fused call share; 1: nothing to do
static int cfg_check(const char* who, int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction,
                     const int32_t* levels, const double* rows_out, const uint8_t* source_out) {
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "%s: D=%d outside [1, %d]", who, D, HBX_MAX_D);
  if (B < 0 || S < 0 || C < 1)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld S=%lld C=%lld", who, (long long)B, (long long)S, (long long)C);
  if (!grp_counts_ok(B, S, C))  // (what the grids and the slot indices of the composition rely on)
    return hbx_fail(HBX_ERR_ARG, "%s: B * S * C = %lld * %lld * %lld exceeds int32", who, (long long)B, (long long)S,
                    (long long)C);
  if (!(random_fraction >= 0.0 && random_fraction <= 1.0))
    return hbx_fail(HBX_ERR_ARG, "%s: random_fraction=%g outside [0, 1]", who, random_fraction);
  if (B == 0 || S == 0) return 1;
  if (!levels || !rows_out || !source_out) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  if ((uintptr_t)rows_out & 7) return hbx_fail(HBX_ERR_ARG, "%s: rows_out must be 8-byte aligned", who);
  return HBX_OK;
}

static int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static int cfg_finish(const char* who, const void* records, const double* cands, const uint8_t* domain_err,
                      const int32_t* levels, int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction,
                      uint64_t seed, uint64_t counter_base, uint32_t stream_id, const uint8_t* want, double* rows_out,
                      uint8_t* source_out, void* stream) {
  const int rc = cfg_check(who, D, B, S, C, random_fraction, levels, rows_out, source_out);
  if (rc) return rc < 0 ? rc : HBX_OK;
  if (records && !cands) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (cands)", who);
  if (((uintptr_t)records & 7) || ((uintptr_t)cands & 7))
    return hbx_fail(HBX_ERR_ARG, "%s: records and cands must be 8-byte aligned", who);
  const int64_t Q = B * S;
  hipLaunchKernelGGL(want ? groups_finish_kernel<true> : groups_finish_kernel<false>,
                     dim3((unsigned)((Q + FIN_WAVES - 1) / FIN_WAVES)), dim3(64 * FIN_WAVES), 0, (hipStream_t)stream,
                     (const AcqResult*)records, cands, records ? domain_err : nullptr, levels, D, Q, C, random_fraction,
                     seed, counter_base, stream_id, rows_out, source_out, want);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

int hbx_kde_finish_groups(const void* records, const double* cands, const uint8_t* domain_err, const int32_t* levels,
                          int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                          uint64_t counter_base, uint32_t stream_id, double* rows_out, uint8_t* source_out,
                          void* stream) {
  return cfg_finish("hbx_kde_finish_groups", records, cands, domain_err, levels, D, B, S, C, random_fraction, seed,
                    counter_base, stream_id, nullptr, rows_out, source_out, stream);
}

int hbx_kde_finish_groups_m(const void* records, const double* cands, const uint8_t* domain_err, const int32_t* levels,
                            int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                            uint64_t counter_base, uint32_t stream_id, const uint8_t* want, double* rows_out,
                            uint8_t* source_out, void* stream) {
  return cfg_finish("hbx_kde_finish_groups_m", records, cands, domain_err, levels, D, B, S, C, random_fraction, seed,
                    counter_base, stream_id, want, rows_out, source_out, stream);
}

int hbx_kde_random_requests_groups(int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                                   uint64_t counter_base, uint32_t stream_id, const uint8_t* want_in, uint8_t* want_out,
                                   void* stream) {
  const char* who = "hbx_kde_random_requests_groups";
  if (B < 0 || S < 0 || C < 1)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld S=%lld C=%lld", who, (long long)B, (long long)S, (long long)C);
  if (!grp_counts_ok(B, S, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * S * C = %lld * %lld * %lld exceeds int32", who, (long long)B, (long long)S,
                    (long long)C);
  if (!(random_fraction >= 0.0 && random_fraction <= 1.0))
    return hbx_fail(HBX_ERR_ARG, "%s: random_fraction=%g outside [0, 1]", who, random_fraction);
  if (B == 0 || S == 0) return HBX_OK;
  if (!want_out) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (want_out)", who);
  const int64_t Q = B * S;
  hipLaunchKernelGGL(groups_random_requests_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     Q, C, random_fraction, seed, counter_base, stream_id, want_in, want_out);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// the fused call's workspace: [the batched acquisition's][pools f64 B S C D][error bytes B S C][records B S 48]
int hbx_kde_propose_groups_ws_offsets(int64_t B, int64_t S, int64_t C, int32_t D, int64_t* out4) {
  if (!out4) return hbx_fail(HBX_ERR_ARG, "hbx_kde_propose_groups_ws_offsets: null pointer");
  const int64_t acq = C < 1 ? -1 : hbx_kde_groups_batch_workspace_bytes(B, S, C, D);
  if (acq < 0)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_propose_groups_ws_offsets: B=%lld S=%lld C=%lld D=%d out of range",
                    (long long)B, (long long)S, (long long)C, D);
  const int64_t P = B * S * C;
  out4[0] = align16(acq);                              // pools
  out4[1] = out4[0] + align16(P * (int64_t)D * 8);      // error bytes
  out4[2] = out4[1] + align16(P);                      // records
  out4[3] = out4[2] + align16(B * S * (int64_t)sizeof(AcqResult));  // the end
  return HBX_OK;
}

int64_t hbx_kde_propose_groups_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D) {
  int64_t off[4];
  return hbx_kde_propose_groups_ws_offsets(B, S, C, D, off) == HBX_OK ? off[3] : -1;
}

int hbx_kde_propose_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                           const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                           const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad,
                           const int32_t* levels, double bandwidth_factor, double random_fraction, uint64_t seed,
                           uint64_t counter_base, uint32_t stream_id, int64_t S, int64_t C, double* rows_out,
                           uint8_t* source_out, void* records_out, double* cands_out, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return hbx_kde_propose_groups_r(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad,
                                  levels, bandwidth_factor, random_fraction, seed, counter_base, stream_id, S, C,
                                  rows_out, source_out, records_out, cands_out, workspace, workspace_bytes, stream,
                                  nullptr);
}

// the composition with hbx_kde_acquire_groups_batch_r in the middle: the requests' scores under rules->pdf_floor
int hbx_kde_propose_groups_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                             const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                             const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad,
                             const int32_t* levels, double bandwidth_factor, double random_fraction, uint64_t seed,
                             uint64_t counter_base, uint32_t stream_id, int64_t S, int64_t C, double* rows_out,
                             uint8_t* source_out, void* records_out, double* cands_out, void* workspace,
                             int64_t workspace_bytes, void* stream, const hbx_rules* rules) {
  const char* who = rules ? "hbx_kde_propose_groups_r" : "hbx_kde_propose_groups";
  if (const int rrc = hbx_rules_check(who, rules)) return rrc;
  const int rc = cfg_check(who, D, B, S, C, random_fraction, levels, rows_out, source_out);
  if (rc) return rc < 0 ? rc : HBX_OK;
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !bw_good || !bw_bad || !nlev_good || !nlev_bad ||
      !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  int64_t off[4];
  if (hbx_kde_propose_groups_ws_offsets(B, S, C, D, off) != HBX_OK) return HBX_ERR_ARG;
  if (workspace_bytes < off[3])
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)workspace_bytes,
                    (long long)off[3]);
  if (((uintptr_t)workspace & 15) || ((uintptr_t)records_out & 7) || ((uintptr_t)cands_out & 7))
    return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte, records_out and cands_out 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* pool = (double*)(ws + off[0]);
  uint8_t* err = (uint8_t*)(ws + off[1]);
  void* rec = records_out ? records_out : (void*)(ws + off[2]);  // written in place: no copy on the default path
  int r = hbx_kde_sample_groups(X, D, seg_off, B, order, n_good, bw_good, levels, bandwidth_factor, seed, counter_base,
                                stream_id, S * C, pool, err, stream);
  if (r != HBX_OK) return r;
  r = hbx_kde_acquire_groups_batch_r(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good,
                                     nlev_bad, pool, S, C, rec, workspace, off[0], stream, rules);
  if (r != HBX_OK) return r;
  r = hbx_kde_finish_groups(rec, pool, err, levels, D, B, S, C, random_fraction, seed, counter_base, stream_id,
                            rows_out, source_out, stream);
  if (r != HBX_OK) return r;
  if (cands_out)  // (a diagnostic output: the pools stay in the workspace either way)
    HBX_HIP(hipMemcpyAsync(cands_out, pool, (size_t)(B * S * C) * (size_t)D * 8, hipMemcpyDeviceToDevice, s));
  return HBX_OK;
}

// the masked call's workspace: hbx_kde_propose_groups' followed by the effective mask u8[B][S]
int hbx_kde_propose_groups_m_ws_offsets(int64_t B, int64_t S, int64_t C, int32_t D, int64_t* out5) {
  if (!out5) return hbx_fail(HBX_ERR_ARG, "hbx_kde_propose_groups_m_ws_offsets: null pointer");
  const int rc = hbx_kde_propose_groups_ws_offsets(B, S, C, D, out5);
  if (rc != HBX_OK) return rc;
  out5[4] = out5[3] + align16(B * S);  // [3]: the mask, [4]: the end
  return HBX_OK;
}

int64_t hbx_kde_propose_groups_m_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D) {
  int64_t off[5];
  return hbx_kde_propose_groups_m_ws_offsets(B, S, C, D, off) == HBX_OK ? off[4] : -1;
}

int hbx_kde_propose_groups_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                             const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype, const double* bw_good,
                             const double* bw_bad, const int32_t* nlev_good, const int32_t* nlev_bad,
                             const int32_t* levels, double bandwidth_factor, double random_fraction, uint64_t seed,
                             uint64_t counter_base, uint32_t stream_id, int64_t S, int64_t C, const uint8_t* want,
                             int32_t flags, double* rows_out, uint8_t* source_out, void* records_out, double* cands_out,
                             void* workspace, int64_t workspace_bytes, void* stream, const hbx_rules* rules) {
  const char* who = "hbx_kde_propose_groups_m";
  if (const int rrc = hbx_rules_check(who, rules)) return rrc;
  if (flags & ~HBX_PROPOSE_SKIP_RANDOM) return hbx_fail(HBX_ERR_ARG, "%s: flags=%d", who, flags);
  const int rc = cfg_check(who, D, B, S, C, random_fraction, levels, rows_out, source_out);
  if (rc) return rc < 0 ? rc : HBX_OK;
  if (!X || !seg_off || !order || !n_good || !n_bad || !vartype || !bw_good || !bw_bad || !nlev_good || !nlev_bad ||
      !workspace)
    return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  int64_t off[5];
  if (hbx_kde_propose_groups_m_ws_offsets(B, S, C, D, off) != HBX_OK) return HBX_ERR_ARG;
  if (workspace_bytes < off[4])
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)workspace_bytes,
                    (long long)off[4]);
  if (((uintptr_t)workspace & 15) || ((uintptr_t)records_out & 7) || ((uintptr_t)cands_out & 15))
    return hbx_fail(HBX_ERR_ARG, "%s: workspace and cands_out must be 16-byte, records_out 8-byte aligned", who);
  char* ws = (char*)workspace;
  // cands_out, when given, is the pool itself: an unwanted request's rows are then not written there either
  double* pool = cands_out ? cands_out : (double*)(ws + off[0]);
  uint8_t* err = (uint8_t*)(ws + off[1]);
  void* rec = records_out ? records_out : (void*)(ws + off[2]);
  const uint8_t* eff = want;  // what the sampler and the acquisition answer
  if (flags & HBX_PROPOSE_SKIP_RANDOM) {
    uint8_t* m = (uint8_t*)(ws + off[3]);
    const int r = hbx_kde_random_requests_groups(B, S, C, random_fraction, seed, counter_base, stream_id, want, m, stream);
    if (r != HBX_OK) return r;
    eff = m;
  }
  int r = hbx_kde_sample_groups_m(X, D, seg_off, B, order, n_good, bw_good, levels, bandwidth_factor, seed, counter_base,
                                  stream_id, S, C, eff, pool, err, stream);
  if (r != HBX_OK) return r;
  r = hbx_kde_acquire_groups_batch_m(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good,
                                     nlev_bad, pool, S, C, eff, rec, workspace, off[0], stream, rules);
  if (r != HBX_OK) return r;
  return want ? hbx_kde_finish_groups_m(rec, pool, err, levels, D, B, S, C, random_fraction, seed, counter_base,
                                        stream_id, want, rows_out, source_out, stream)
              : hbx_kde_finish_groups(rec, pool, err, levels, D, B, S, C, random_fraction, seed, counter_base,
                                      stream_id, rows_out, source_out, stream);
}

}  // extern "C"
