// hbx_score.hip -- scoring dispatch on MI355X (gfx950): which fp32 scoring instance a prepared KDE runs
// (hbx_score_f32 / _oh / _h / _h32.hip hold them), the launch of one KDE's or a pair's scoring with its rescue
// pass, and the rescue kernels.  hbx_kde_logpdf scores candidates against one KDE; the acquisitions
// (hbx_kde.hip, hbx_topk.hip) launch through launch_score2.
#include "hbx_score.h"

#include <hip/hip_ext.h>

#include "hbx_prep.h"
#include "hbx_rescue_impl.h"

template <int DCP, bool SIGNED>
__device__ __forceinline__ void kde_rescue_body(const double* __restrict__ cand, int64_t Nc, int32_t D,
                                                const KdeParams* __restrict__ P, const float* __restrict__ table,
                                                KdeEst* __restrict__ out, const unsigned blk,
                                                const int nsplit = 1) {
  const int64_t i = (int64_t)blk * 256 + threadIdx.x;
  bool need = false;  // a marker in any observation split's partial estimate
  if (i < Nc)
    for (int r = 0; r < nsplit; ++r) need = need || out[(int64_t)r * Nc + i].err == -1.f;
  if (!__any(need)) return;
  if (!need) return;
  out[i] = kde_rescue_one<DCP, SIGNED>(cand, i, D, P);  // the whole sum in split 0
  for (int r = 1; r < nsplit; ++r) out[(int64_t)r * Nc + i] = kde_est_neutral();
}

template <int DCP, bool SIGNED>
__global__ __launch_bounds__(256) void kde_rescue_kernel(const double* __restrict__ cand, int64_t Nc, int32_t D,
                                                         const KdeParams* __restrict__ P,
                                                         const float* __restrict__ table,
                                                         KdeEst* __restrict__ out) {
  kde_rescue_body<DCP, SIGNED>(cand, Nc, D, P, table, out, blockIdx.x);
}


// both KDEs' rescue passes in one launch (blocks [0, nblk0) KDE 0, the rest KDE 1)
// grid-stride over the 2 nblk0 logical blocks; with the scoring kernel's marker count available and 0
// (the common case) every workgroup exits after one load; its first
// workgroup also initialises a single acquisition's state (acq_init's work)
template <int DCP, bool SIGNED>
__global__ __launch_bounds__(256) void kde_rescue_pair_kernel(const double* __restrict__ cand, int64_t Nc, int32_t D,
                                                              KdePairArgs a) {
  if (a.init.U && blockIdx.x == 0 && threadIdx.x == 0)  // a single acquisition's state (acq_init's work)
    acq_init_state(a.init.U, a.init.count, a.init.flags, a.init.first1, a.init.res);
  if (a.rescue && __hip_atomic_load(a.rescue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  for (unsigned b = blockIdx.x; b < 2 * a.nblk0; b += gridDim.x) {
    const bool second = b >= a.nblk0;
    kde_rescue_body<DCP, SIGNED>(cand, Nc, D, second ? a.P1 : a.P0, second ? a.table1 : a.table0,
                                 second ? a.out1 : a.out0, second ? b - a.nblk0 : b, second ? a.nsplit1 : a.nsplit0);
  }
}

// ------------------------------------------------------------------------------------------
// launch-side dispatch over the (dc_pad, du_pad, signed) template buckets

// Observation splits of a pair launch with `tiles` candidate tiles per KDE over <= nmax observations: a
// few candidates against many observations would otherwise be a handful of blocks each walking every
// chunk (64 candidates x 1e4 observations: 2 blocks, 123 us); while both KDEs' tiles are at most one block
// per CU, split until they fill the chip about twice, each range >= 4 chunks, at most 16 (the combine
// kernel merges the partial sums).
// HBX_OBS_SPLIT=0: no splits (read per call).  ws_sizing: the workspace's bound (no switch, the largest
// tile size).
int obs_splits(unsigned tiles, int64_t nmax, bool ws_sizing) {
  if (!ws_sizing && !hbx_switch_on("HBX_OBS_SPLIT")) return 1;
  const int64_t nch = (nmax + OBS_CHUNK - 1) / OBS_CHUNK;
  if (2 * (int64_t)tiles > 256) return 1;  // one block per CU or more already (config #2: 392 blocks; both
                                           // KDEs split in two measured 4 us slower: a second round)
  int64_t sp = (512 + 2 * (int64_t)tiles - 1) / (2 * (int64_t)(tiles > 0 ? tiles : 1));
  if (sp > nch / 4) sp = nch / 4;
  if (sp > OBS_SPLIT_MAX) sp = OBS_SPLIT_MAX;
  return sp < 1 ? 1 : (int)sp;
}

template <bool SG>
static logpdf_pair_fn pick_rescue_pair(int dc_pad) {
  switch (dc_pad) {
    case 0: return kde_rescue_pair_kernel<0, SG>;
    case 4: return kde_rescue_pair_kernel<4, SG>;
    case 8: return kde_rescue_pair_kernel<8, SG>;
    case 16: return kde_rescue_pair_kernel<16, SG>;
    case 24: return kde_rescue_pair_kernel<24, SG>;
    case 32: return kde_rescue_pair_kernel<32, SG>;
    case 64: return kde_rescue_pair_kernel<64, SG>;
  }
  return nullptr;
}

template <bool SG>
static logpdf_fn pick_rescue(int dc_pad) {
  switch (dc_pad) {
    case 0: return kde_rescue_kernel<0, SG>;
    case 4: return kde_rescue_kernel<4, SG>;
    case 8: return kde_rescue_kernel<8, SG>;
    case 16: return kde_rescue_kernel<16, SG>;
    case 24: return kde_rescue_kernel<24, SG>;
    case 32: return kde_rescue_kernel<32, SG>;
    case 64: return kde_rescue_kernel<64, SG>;
  }
  return nullptr;
}

// (the variant code and `fast`: hbx_score.h)
ScoreFns pick_logpdf(int dc_pad, int du_pad, int variant, bool fast) {
  const bool sg = variant & 1;
  const int kc = du_pad == 0 ? 0 : (variant >> 1) & 7;  // no categorical dims: kc irrelevant
  const bool hm = (variant >> 4) & 1;
  int dcp, dup;
  bucket_dims(dc_pad, du_pad, &dcp, &dup);
  if (dcp != dc_pad || dup != du_pad) return {nullptr, nullptr, 0, 0, nullptr, nullptr};  // not a bucket
  const logpdf_fn r = sg ? pick_rescue<true>(dc_pad) : pick_rescue<false>(dc_pad);
  if (hm && ((variant >> 6) & 1)) {
    if (dc_pad < 8) return {nullptr, nullptr, 0, 0, nullptr, nullptr};
    const int kp = h32_kp(kc);
    const bool co = fast && !sg && ((variant >> 7) & 1);  // the acquisition's coarse pre-screen instance
    const bool fa = fast && kp > 0;
    const int hw = co ? H32C_WAVES : H16_WAVES;
    ScoreFns f{hbx_pick_h32(nsc_of(dc_pad), kp, sg, fa, co), r, 32 * hw * (co ? H32C_CT : 1), 64 * hw,
               hbx_pick_h32_pair(nsc_of(dc_pad), kp, sg, fa, co),
               sg ? pick_rescue_pair<true>(dc_pad) : pick_rescue_pair<false>(dc_pad), true};
    if (co && H32C_CT > 1) f.pair1 = hbx_pick_h32_pair1(nsc_of(dc_pad), kp);
    if (co) f.list = hbx_pick_h32_list(nsc_of(dc_pad), kp);
    return f;
  }
  if (hm) {
    if (dc_pad < 8) return {nullptr, nullptr, 0, 0, nullptr, nullptr};
    return {hbx_pick_h(nsc_of(dc_pad), kc, sg), r, 16 * H16_WAVES * H_ROW_TILES, 64 * H16_WAVES,
            hbx_pick_h_pair(nsc_of(dc_pad), kc, sg), sg ? pick_rescue_pair<true>(dc_pad) : pick_rescue_pair<false>(dc_pad)};
  }
  if (kc == 0) return {hbx_pick_f32(dc_pad, du_pad, sg), r, 16 * MFMA_WAVES, 64 * MFMA_WAVES, nullptr, nullptr};
  return {hbx_pick_oh(dc_pad, kc, sg), r, 16 * MFMA_WAVES, 64 * MFMA_WAVES, nullptr, nullptr};
}

int launch_score(ScoreFns f, const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                 KdeEst* est, hipStream_t s) {
  const unsigned gm = (unsigned)((Nc + f.cands_per_block - 1) / f.cands_per_block);
  hipLaunchKernelGGL(f.main, dim3(gm), dim3(f.threads), 0, s, cand, Nc, D, (const KdeParams*)params, table, est);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(f.rescue, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, cand, Nc, D,
                     (const KdeParams*)params, table, est);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// (hbx_score.h.)  HBX_SCORE_PAIR=0 keeps two launches; HBX_PAIR1=0 always the H32C_CT-tile coarse pair kernel
// (both read per call: tests switch them in-process)
int launch_score2(ScoreFns f0, const void* params0, const float* table0, KdeEst* est0, ScoreFns f1,
                  const void* params1, const float* table1, KdeEst* est1, const double* cand, int64_t Nc, int32_t D,
                  hipEvent_t* ev, int32_t* rescue_cnt, hipStream_t s, KdePairArgs::AcqInitPtrs init, bool* inited,
                  int64_t nmax, int32_t* nsplit_out, bool* rescue_inline) {
  if (nsplit_out) nsplit_out[0] = nsplit_out[1] = 1;
  if (rescue_inline) *rescue_inline = false;
  const bool pair = f0.pair && f0.main == f1.main && f0.rescue_pair && f0.rescue == f1.rescue &&
                    hbx_switch_on("HBX_SCORE_PAIR");
  if (ev && !pair) HBX_HIP(hipEventRecord(ev[0], s));
  if (pair) {
    unsigned gm = (unsigned)((Nc + f0.cands_per_block - 1) / f0.cands_per_block);
    logpdf_pair_fn pk = f0.pair;
    // both KDEs' blocks within one round of the chip's slots (two per CU): one column tile per wave instead,
    // twice the waves (config #2: 52 instead of 53.5 us per acquisition; profiles/r06/ct1/)
    if (f0.pair1 && f0.pair1 == f1.pair1 && 2 * gm <= 512 && hbx_switch_on("HBX_PAIR1")) {
      pk = f0.pair1;
      gm = (unsigned)((Nc + f0.cands_per_block / H32C_CT - 1) / (f0.cands_per_block / H32C_CT));
    }
    const unsigned gr = (unsigned)((Nc + 255) / 256);
    if ((uint64_t)gr * 2 > 0x7fffffffu) return hbx_fail(HBX_ERR_ARG, "too many candidates for one pair launch");
    const bool can = f0.split_ok && nsplit_out && nmax > 0;
    // segment 0 = params1 (the bad KDE), 1 = params0.  (At about one block per CU -- config #2, 2 x 196
    // blocks -- splitting only the bad KDE's longer walks in two measured 3-5 us slower, like splitting
    // both: each range repeats the block's prologue, and the merge reads twice the estimates.)
    const int ns0 = can ? obs_splits(gm, nmax) : 1, ns1 = ns0;
    KdePairArgs a{(const KdeParams*)params1, (const KdeParams*)params0, table1, table0, est1, est0, gm * ns0,
                  rescue_cnt, {}};
    a.tiles = gm;
    a.nsplit0 = ns0;
    a.nsplit1 = ns1;
    if (nsplit_out) {
      nsplit_out[0] = ns1;  // params0's (the first KDE argument's) splits
      nsplit_out[1] = ns0;
    }
    const unsigned grid = gm * (unsigned)(ns0 + ns1);
    const bool pinit = f0.split_ok && HBX_PAIR_INIT;
    if (pinit) a.init = init;  // the 32x32 pair kernel's first workgroup sets the acquisition state
    if (ev)  // events stamped by the dispatch itself at the kernel's start and end (rocprof's duration)
      hipExtLaunchKernelGGL(pk, dim3(grid), dim3(f0.threads), 0, s, ev[0], ev[1], 0, cand, Nc, D, a);
    else
      hipLaunchKernelGGL(pk, dim3(grid), dim3(f0.threads), 0, s, cand, Nc, D, a);
    HBX_LAUNCH_CHECK();
    a.nblk0 = gr;
    a.init = pinit ? KdePairArgs::AcqInitPtrs{} : init;  // else set by the rescue pass's first workgroup
    if (inited) *inited = init.U != nullptr;
    if (rescue_inline && pinit && rescue_cnt && ns0 == 1 && ns1 == 1) {
      *rescue_inline = true;  // the combine kernel (kde_combine_kernel<signed, true>) re-scores the marked candidates
      return HBX_OK;
    }
    // the rescue pass: grid-stride, exits at once unless the scoring kernel counted a marker
    const unsigned grr = rescue_cnt ? (2 * gr < 1024u ? 2 * gr : 1024u) : 2 * gr;
    hipLaunchKernelGGL(f0.rescue_pair, dim3(grr), dim3(256), 0, s, cand, Nc, D, a);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  int rc = launch_score(f0, cand, Nc, D, params0, table0, est0, s);
  if (rc) return rc;
  if (ev) HBX_HIP(hipEventRecord(ev[1], s));
  rc = launch_score(f1, cand, Nc, D, params1, table1, est1, s);
  if (rc) return rc;
  if (ev) HBX_HIP(hipEventRecord(ev[2], s));
  return HBX_OK;
}

extern "C" {

// fp32 log-domain scoring of Nc candidates (fp64 [Nc][D] row-major) against one prepared KDE
int hbx_kde_logpdf(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                   int32_t dc_pad, int32_t du_pad, int32_t variant, void* est_out, void* stream) {
  if ((!cand || !est_out) && Nc > 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf: null pointer");
  if (!params || !table) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf: null pointer");
  if (Nc <= 0) return HBX_OK;
  ScoreFns f = pick_logpdf(dc_pad, du_pad, variant);
  if (!f.main) return hbx_fail(HBX_ERR_UNSUPPORTED, "no kernel for dc_pad=%d du_pad=%d", dc_pad, du_pad);
  return launch_score(f, cand, Nc, D, params, table, (KdeEst*)est_out, (hipStream_t)stream);
}

}  // extern "C"

int hbx_logpdf_estimate(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                        int32_t dc_pad, int32_t du_pad, int32_t variant, KdeEst* est, hipStream_t s) {
  ScoreFns f = pick_logpdf(dc_pad, du_pad, variant);
  if (!f.main) return hbx_fail(HBX_ERR_UNSUPPORTED, "no kernel for dc_pad=%d du_pad=%d", dc_pad, du_pad);
  return launch_score(f, cand, Nc, D, params, table, est, s);
}
