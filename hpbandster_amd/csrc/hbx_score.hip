// hbx_score.hip -- scoring dispatch on MI355X (gfx950): which fp32 scoring instance a prepared KDE runs
// (hbx_score_f32 / _oh / _h / _h32.hip hold them: each picks its instance for a bucket through the one ladder of
// hbx_pick.h and hands it back with the block it is compiled for, so no launch shape is restated here), the launch
// of one KDE's or a pair's scoring with its rescue pass, and the rescue kernels.  hbx_kde_logpdf scores candidates against one KDE; the acquisitions
// (hbx_kde.hip acq_score, and through it hbx_topk.hip) launch through launch_score2; pair_shape is the one rule for
// a pair launch's kernel, tiles and splits (the fused launch here, stage 1 of hbx_staged.hip).
#include "hbx_score.h"

#include <hip/hip_ext.h>

#include "hbx_pick.h"
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

// observation splits of a list launch: lists are short (tens of candidates, one or two tiles), so as many
// ranges as leave each >= 4 chunks -- 16 at the bench's 8500 bad observations: one tile's 16 blocks of 8 chunks
int list_splits(int64_t nmax) {
  if (!hbx_switch_on("HBX_OBS_SPLIT")) return 1;
  const int64_t sp = ((nmax + OBS_CHUNK - 1) / OBS_CHUNK) / 4;
  return sp < 1 ? 1 : sp > OBS_SPLIT_MAX ? OBS_SPLIT_MAX : (int)sp;
}

// (hbx_score.h)
PairShape pair_shape(const ScoreFns& f, bool pair1_ok, int kdes, int64_t Nc, int64_t split_nmax) {
  PairShape sh{f.pair, (unsigned)((Nc + f.cands_per_block - 1) / f.cands_per_block), 1};
  // every block of the launch within one round of the chip's slots (two per CU): one column tile per wave
  // instead, twice the waves (config #2: 52 instead of 53.5 us per acquisition; profiles/r06/ct1/).  The fused
  // launch's rule is 2 tiles <= 512 because both KDEs' blocks share the slots; stage 1 of the staged acquisition
  // has them to itself, so tiles <= 512.  Measured there with HBX_PAIR1=1 / 0 under HBX_STAGED=2
  // (profiles/staged/onoff_pair1.jsonl): the staged call is 8 % faster with it at 1.4e5 candidates and equal at
  // 2.0e5 and 2.6e5.
  if (pair1_ok && f.pair1 && (unsigned)kdes * sh.tiles <= 512 && hbx_switch_on("HBX_PAIR1")) {
    sh.kernel = f.pair1;
    sh.tiles = (unsigned)((Nc + f.cands_per_block / H32C_CT - 1) / (f.cands_per_block / H32C_CT));
  }
  // (At about one block per CU -- config #2, 2 x 196 blocks -- splitting only the bad KDE's longer walks in two
  // measured 3-5 us slower, like splitting both: each range repeats the block's prologue, and the merge reads
  // twice the estimates.  So one split count for every KDE of the launch.)
  if (f.split_ok && split_nmax > 0) sh.nsplit = obs_splits(sh.tiles, split_nmax, false);
  return sh;
}

static const ScoreFns NO_SCORE_FNS{nullptr, nullptr, 0, 0, nullptr, nullptr};  // no instance for the bucket

// (the variant code and `fast`: hbx_score.h)  The family's file picks the instance and says what block it is
// compiled for; here: which family a variant runs, the rescue kernels of its bucket, and what the coarse
// instances need around them.
ScoreFns pick_logpdf(int dc_pad, int du_pad, int variant, bool fast) {
  const KdeVariant v = KdeVariant::decode(variant);
  const bool sg = v.has_neg;
  const int kc = du_pad == 0 ? 0 : v.kc;  // no categorical dims: kc irrelevant
  int dcp, dup;
  bucket_dims(dc_pad, du_pad, &dcp, &dup);
  if (dcp != dc_pad || dup != du_pad) return NO_SCORE_FNS;  // not a bucket
  struct Rescue {
    logpdf_fn one;
    logpdf_pair_fn pair;
  };
  const Rescue r = hbx_pick<0, 1>(sg, [=](auto s) {
    return hbx_pick<0, 4, 8, 16, 24, 32, 64>(dc_pad, [](auto dc) {
      return Rescue{kde_rescue_kernel<HBX_PICKED(dc), HBX_PICKED(s) != 0>,
                    kde_rescue_pair_kernel<HBX_PICKED(dc), HBX_PICKED(s) != 0>};
    });
  });
  if (v.hmode && dc_pad < 8) return NO_SCORE_FNS;
  if (v.hmode && v.h32) {
    const int kp = h32_kp(kc);
    const bool co = fast && !sg && v.coarse;  // the acquisition's coarse pre-screen instance
    const H32Inst h = hbx_pick_h32(nsc_of(dc_pad), kp, sg, fast && kp > 0, co);
    ScoreFns f{h.main, r.one, h.cands_per_block, h.threads, h.pair, r.pair, true};
    if (co && H32C_CT > 1) f.pair1 = h.pair1;
    if (co) f.list = h.list;
    if (co) f.main_co = h.main_co;
    if (co && !f.main_co) return NO_SCORE_FNS;
    return f;
  }
  // the 16x16 hmode family; else the f32 families (no pair launch): categorical match on the VALU, or one-hot
  const ScoreInst k = v.hmode ? hbx_pick_h(nsc_of(dc_pad), kc, sg)
                              : kc == 0 ? hbx_pick_f32(dc_pad, du_pad, sg) : hbx_pick_oh(dc_pad, kc, sg);
  return {k.main, r.one, k.cands_per_block, k.threads, k.pair, v.hmode ? r.pair : nullptr};
}

int launch_score(ScoreFns f, const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                 KdeEst* est, hipStream_t s) {
  const unsigned gm = (unsigned)((Nc + f.cands_per_block - 1) / f.cands_per_block);
  if (f.main_co)
    hipLaunchKernelGGL(f.main_co, dim3(gm), dim3(f.threads), 0, s, cand, Nc, D, (const KdeParams*)params, table, est,
                       hbx_row_stage());
  else
    hipLaunchKernelGGL(f.main, dim3(gm), dim3(f.threads), 0, s, cand, Nc, D, (const KdeParams*)params, table, est);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(f.rescue, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, cand, Nc, D,
                     (const KdeParams*)params, table, est);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// (hbx_score.h.)  HBX_SCORE_PAIR=0 keeps two launches (read per call: tests switch it in-process)
int launch_score2(const ScoreSide& good, const ScoreSide& bad, const ScoreRequest& rq, ScoreResult* out) {
  *out = ScoreResult{};
  const ScoreFns& f = good.f;
  const hipStream_t s = rq.s;
  const bool pair = f.pair && f.main == bad.f.main && f.main_co == bad.f.main_co && f.rescue_pair &&
                    f.rescue == bad.f.rescue && hbx_switch_on("HBX_SCORE_PAIR");
  if (!pair) {
    if (rq.ev) HBX_HIP(hipEventRecord(rq.ev[0], s));
    int rc = launch_score(f, rq.cand, rq.Nc, rq.D, good.params, good.table, good.est, s);
    if (rc) return rc;
    if (rq.ev) HBX_HIP(hipEventRecord(rq.ev[1], s));
    rc = launch_score(bad.f, rq.cand, rq.Nc, rq.D, bad.params, bad.table, bad.est, s);
    if (rc) return rc;
    if (rq.ev) HBX_HIP(hipEventRecord(rq.ev[2], s));
    return HBX_OK;
  }
  const PairShape sh = pair_shape(f, f.pair1 == bad.f.pair1, 2, rq.Nc, rq.split_nmax);
  const unsigned gr = (unsigned)((rq.Nc + 255) / 256);
  if ((uint64_t)gr * 2 > 0x7fffffffu) return hbx_fail(HBX_ERR_ARG, "too many candidates for one pair launch");
  // segment 0 = the bad KDE, 1 = the good one
  KdePairArgs a{(const KdeParams*)bad.params, (const KdeParams*)good.params, bad.table, good.table, bad.est,
                good.est, sh.tiles * sh.nsplit, rq.rescue_cnt, {}};
  a.tiles = sh.tiles;
  a.nsplit0 = a.nsplit1 = sh.nsplit;
  a.row_stage = hbx_row_stage();
  out->nsplit[0] = out->nsplit[1] = sh.nsplit;
  const unsigned grid = sh.tiles * (unsigned)(2 * sh.nsplit);
  const bool pinit = f.split_ok && HBX_PAIR_INIT;
  if (pinit) a.init = rq.init;  // the 32x32 pair kernel's first workgroup sets the acquisition state
  if (rq.ev)  // events stamped by the dispatch itself at the kernel's start and end (rocprof's duration)
    hipExtLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, rq.ev[0], rq.ev[1], 0, rq.cand, rq.Nc, rq.D, a);
  else
    hipLaunchKernelGGL(sh.kernel, dim3(grid), dim3(f.threads), 0, s, rq.cand, rq.Nc, rq.D, a);
  HBX_LAUNCH_CHECK();
  a.nblk0 = gr;
  a.init = pinit ? KdePairArgs::AcqInitPtrs{} : rq.init;  // else set by the rescue pass's first workgroup
  out->inited = rq.init.U != nullptr;
  if (rq.combine_rescues && pinit && rq.rescue_cnt && sh.nsplit == 1) {
    out->rescue_inline = true;  // the combine kernel (kde_combine_kernel<signed, true>) re-scores the marked candidates
    return HBX_OK;
  }
  // the rescue pass: grid-stride, exits at once unless the scoring kernel counted a marker
  const unsigned grr = rq.rescue_cnt ? (2 * gr < 1024u ? 2 * gr : 1024u) : 2 * gr;
  hipLaunchKernelGGL(f.rescue_pair, dim3(grr), dim3(256), 0, s, rq.cand, rq.Nc, rq.D, a);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

// fp32 log-domain scoring of Nc candidates (fp64 [Nc][D] row-major) against one prepared KDE
int hbx_kde_logpdf(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                   int32_t dc_pad, int32_t du_pad, int32_t variant, void* est_out, void* stream) {
  if ((!cand || !est_out) && Nc > 0) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf: null pointer");
  if (!params || !table) return hbx_fail(HBX_ERR_ARG, "hbx_kde_logpdf: null pointer");
  if (Nc <= 0) return HBX_OK;
  ScoreFns f = pick_logpdf(dc_pad, du_pad, variant, false);
  if (!f.main) return hbx_fail(HBX_ERR_UNSUPPORTED, "no kernel for dc_pad=%d du_pad=%d", dc_pad, du_pad);
  return launch_score(f, cand, Nc, D, params, table, (KdeEst*)est_out, (hipStream_t)stream);
}

}  // extern "C"

int hbx_logpdf_estimate(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                        int32_t dc_pad, int32_t du_pad, int32_t variant, KdeEst* est, hipStream_t s) {
  ScoreFns f = pick_logpdf(dc_pad, du_pad, variant, false);
  if (!f.main) return hbx_fail(HBX_ERR_UNSUPPORTED, "no kernel for dc_pad=%d du_pad=%d", dc_pad, du_pad);
  return launch_score(f, cand, Nc, D, params, table, est, s);
}
