/* hbx.h -- C ABI of libhbx.so, the MI355X (gfx950) engine for HpBandSter's data-parallel hot path:
 * BOHB's KDE acquisition (good/bad product-kernel KDE fit, l(x)/g(x) scoring, argmin) and the
 * successive-halving promotion.
 *
 * Conventions
 *   - Every pointer marked "device" is a HIP device pointer (e.g. torch.Tensor.data_ptr() of a
 *     ROCm tensor); "host" pointers are ordinary CPU memory.  The library allocates nothing
 *     per call: callers own outputs, workspaces and scratch (sized by the *_bytes helpers).
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue work, except
 *     hbx_kde_prepare, which synchronises `stream` once to upload the model parameters.
 *   - Return value 0 on success, a negative HBX_ERR_* code otherwise; the message is available
 *     from hbx_last_error() (thread-local).  Calls are reentrant; nothing is cached globally.
 *
 * Reference interfaces replaced (paths relative to the HpBandSter snapshot):
 *   hbx_seg_argsort(_ex) + hbx_kde_fit <- bohb.py:220-246 (BOHB.new_result refit:
 *                                      np.argsort + sm.nonparametric.KDEMultivariate(..,'normal_reference'))
 *   hbx_kde_refit                   <- bohb.py:211-251 (the same refit plus both KDEs' preparation, one call)
 *   hbx_kde_refit_sync              <- bohb.py:211-251 (the same, the output block on the host when it returns)
 *   hbx_kde_prepare                 <- KDEMultivariate.__init__ model state (statsmodels 0.12.2
 *                                      kernel_density.py:101-115)
 *   hbx_kde_acquire                 <- bohb.py:124-169 (the num_samples loop: pdf of l and g per
 *                                      candidate, minimize_me, strict-'<' argmin)
 *   hbx_kde_acquire_groups          <- bohb.py:124-169 per bracket, after bohb.py:220-246 (B brackets' picks in
 *                                      one call, straight from hbx_kde_fit's device outputs)
 *   hbx_kde_acquire_groups_batch    <- bohb.py:124-169 once per get_config request of a stage, HB_iteration.py:136-138
 *                                      (S requests per bracket, B brackets, one call)
 *   hbx_kde_acquire_groups_topk     <- bohb.py:124-169 per bracket, the scores ranked: the k best candidates of
 *                                      every bracket's pool by (score, index), one call
 *   hbx_kde_sample_groups           <- bohb.py:133-147 per bracket (the candidates of B brackets in one call)
 *   hbx_kde_finish_groups           <- bohb.py:107-111,154-166 per request (the prior draw where get_config does not
 *                                      return a model-based pick; the winning row otherwise), B x S requests
 *   hbx_kde_propose_groups          <- bohb.py:104-169 (get_config whole: sample, score, pick, fall back) for S
 *                                      requests of each of B brackets, one call
 *   hbx_kde_logpdf_groups           <- KDEMultivariate.pdf (kernel_density.py:162-196) of both KDEs of every bracket
 *                                      at every candidate of its pool, as ln pdf within a relative tolerance, one call
 *   hbx_kde_logpdf                  <- KDEMultivariate.pdf (kernel_density.py:162-196), fp32 log domain
 *   hbx_kde_pdf_exact               <- KDEMultivariate.pdf, fp64, reference operation order
 *   hbx_sh_promote(_ex)             <- HB_iteration.py:149-190 (SuccessiveHalving.process_results ranks)
 *   hbx_sh_advance_groups           <- HB_iteration.py:184-188 (the survivors move to the next budget, in config-id
 *                                      order) and :135-138 (new configurations fill the stage), B brackets, one call
 *   hbx_argmax_allreduce            <- bohb.py:150-152 'if val < best' across candidate shards on many GPUs
 *                                      (the reference has no multi-GPU path)
 */
#ifndef HBX_H_
#define HBX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBX_OK 0
#define HBX_ERR_ARG (-1)
#define HBX_ERR_HIP (-2)
#define HBX_ERR_UNSUPPORTED (-3)

/* ---- acquisition rules ----------------------------------------------------------------------
 * Two constants of the reference snapshot that releases of the package changed, as parameters.  Wherever a
 * `const hbx_rules*` is taken, NULL means {1e-8, 0}: the reference snapshot's numerics, which is also what every
 * entry point without the argument computes.
 *   pdf_floor f      the score of a candidate is (g > f ? g : f) / (f > l ? f : l) in fp64 (bohb.py:129 with
 *                    f = 1e-8; Python max(): a NaN g gives f, a NaN l gives NaN).  Everything else of the selection
 *                    -- strict '<' and first index, (score, index) for the top-k, rel, the near-tie rule, the
 *                    flags -- is unchanged, and candidates with both pdfs below f still score exactly f / f = 1.
 *                    An l of +inf scores 0 (NaN when g is +inf too).  Accepted: finite, 1e-100 <= f <= 1.
 *   min_bandwidth m  every fitted bandwidth, continuous or categorical, becomes bw < m ? m : bw
 *                    (np.clip(bw, m, None): NaN stays NaN).  Accepted: finite, m >= 0; 0 changes nothing.
 *                    Range-checked by every rules-taking entry point; the score-forming ones make no other use
 *                    of it.
 * Anything outside the accepted ranges is HBX_ERR_ARG. */
typedef struct {
  double pdf_floor;
  double min_bandwidth;
} hbx_rules;

/* ---- introspection ---------------------------------------------------------------------- */
const char* hbx_last_error(void);
const char* hbx_version(void);
int64_t hbx_kde_param_bytes(void);     /* bytes of one prepared KDE parameter block (device) */
int64_t hbx_kde_param_bw_offset(void); /* byte offset of the KDE's fp64 bandwidths bw[D] in that block */
int64_t hbx_kde_est_bytes(void);       /* bytes per candidate of hbx_kde_logpdf output */
int64_t hbx_acq_result_bytes(void);    /* bytes of the acquisition result record */
int32_t hbx_max_dims(void);            /* largest D accepted */

/* ---- KDE refit (BOHB.new_result) --------------------------------------------------------- */
int64_t hbx_sort_scratch_bytes(int64_t N);

/* Stable argsort of every segment's fp64 losses (np.argsort order: -inf < finite < +inf < NaN,
 * ties by position).  loss: device f64[N]; seg_off: device i64[B+1]; max_seg: host bound on the
 * longest segment; order: device i64[N], positions local to each segment. */
int hbx_seg_argsort(const double* loss, const int64_t* seg_off, int64_t B, int64_t max_seg, int64_t N,
                    int64_t* order, void* scratch, int64_t scratch_bytes, void* stream);

/* Tie order of the sorts (argsort split and promotion ranks).
 *   HBX_ORDER_NUMPY: numpy 1.26.4's default np.argsort on an AVX-512 host -- the order the reference's
 *     np.argsort(losses) (bohb.py:229) and np.argsort(np.argsort(losses)) (HB_iteration.py:180,240) give
 *     tied losses (crashed +inf runs, quantised losses): the vendored x86-simd-sort avx512_argsort
 *     <double> restated on the device (hpbandster_amd/csrc/hbx_npsort.h; oracle/np_argsort.py pinned
 *     by numpy's own outputs).  Segments without ties cost one check pass over the sorted order.
 *   HBX_ORDER_STABLE: ties by position. */
#define HBX_ORDER_NUMPY 0
#define HBX_ORDER_STABLE 1

/* hbx_seg_argsort with the tie order chosen (hbx_seg_argsort itself = HBX_ORDER_STABLE); scratch:
 * hbx_sort_scratch_bytes(N). */
int hbx_seg_argsort_ex(const double* loss, const int64_t* seg_off, int64_t B, int64_t max_seg, int64_t N,
                       int64_t* order, void* scratch, int64_t scratch_bytes, int32_t order_mode, void* stream);

/* Normal-reference bandwidths and observed level counts of the good (head n_good of the argsort)
 * and bad (tail n_bad) rows of every segment, bit-exact with numpy's np.std.
 * X: device f64[N][D]; order: from hbx_seg_argsort; n_good/n_bad: device i64[B] (0 = skip);
 * fac_good/fac_bad: device f64[B] = n**(-1/(4+D)) computed on the host with pow();
 * vartype: device i32[D] (0 = continuous, 1 = categorical).
 * Outputs: bw_* device f64[B][D]; nlev_* device i32[B][D] (-1 = categorical code not an
 * integer in [0, 1024)). */
int hbx_kde_fit(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                const int64_t* n_good, const int64_t* n_bad, const double* fac_good, const double* fac_bad,
                const int32_t* vartype, double* bw_good, double* bw_bad, int32_t* nlev_good, int32_t* nlev_bad,
                void* stream);

/* hbx_kde_fit with every fitted bandwidth, continuous or categorical, clipped from below where it is stored:
 * bw < rules->min_bandwidth ? rules->min_bandwidth : bw (hbx_rules, above; NULL: hbx_kde_fit itself). */
int hbx_kde_fit_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                  const int64_t* n_good, const int64_t* n_bad, const double* fac_good, const double* fac_bad,
                  const int32_t* vartype, double* bw_good, double* bw_bad, int32_t* nlev_good, int32_t* nlev_bad,
                  void* stream, const hbx_rules* rules);

/* One-call refit of one budget's KDE pair (bohb.py:211-251: append the new observation(s), np.argsort
 * of the losses, good = head n_good / bad = tail n_bad rows, KDEMultivariate(.., 'normal_reference') for
 * both), enqueued on `stream` without host synchronisation; the caller reads `out` back once.
 *   X / loss: device f64[cap][D] / f64[cap] holding the budget's rows 0..n-1 after the call: rows
 *     n-n_new .. n-1 are copied in from `staged` (device f64[n_new*D + n_new]: rows, then losses;
 *     n_new = 0: X / loss are complete already).
 *   vartype: host i32[D] (0 = continuous, 1 = categorical); n_good / n_bad (bohb.py:224-225, clipped to
 *     n) and fac_* = n_good**(-1/(4+D)) / n_bad**(...) from the host's pow().
 *   params_* / table_*: as hbx_kde_prepare (tables of hbx_kde_table_floats(n_good|n_bad, ...) floats).
 *   out: device, hbx_kde_refit_out_bytes(n, D) bytes = order i64[n] | bw_good f64[D] | bw_bad f64[D] |
 *     nlev_good i32[D] | nlev_bad i32[D] | info_good i32[8] | info_bad i32[8] (info as hbx_kde_prepare);
 *     the KDEs' rows are order[0..n_good) and order[n-n_bad..n) -- keep `out` alive with the model.
 *     The argsort is numpy's (HBX_ORDER_NUMPY): tied losses give the reference's rows, in its order.
 *   scratch: device, hbx_kde_refit_scratch_bytes(n, D) bytes. */
int64_t hbx_kde_refit_out_bytes(int64_t n, int32_t D);
int64_t hbx_kde_refit_scratch_bytes(int64_t n, int32_t D);
int hbx_kde_refit(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype, const double* staged,
                  int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good, double fac_bad, void* params_good,
                  float* table_good, int64_t table_good_floats, void* params_bad, float* table_bad,
                  int64_t table_bad_floats, void* out, void* scratch, int64_t scratch_bytes, void* stream);
/* hbx_kde_refit with the rules' min_bandwidth applied where the fit stores the bandwidths: the output block, both
 * parameter blocks and tables, and with them the samplers and the exact re-score, hold the clipped values.  A
 * categorical dim whose set shows ONE level gets h = min_bandwidth > 0 there; it is modelled (hbx_kde_prepare's
 * variant bit 5: every candidate decided by the fp64 evaluation, match factor 1 - h, mismatch factor the IEEE
 * h / 0 = +inf).  NULL: hbx_kde_refit itself. */
int hbx_kde_refit_r(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype, const double* staged,
                    int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good, double fac_bad, void* params_good,
                    float* table_good, int64_t table_good_floats, void* params_bad, float* table_bad,
                    int64_t table_bad_floats, void* out, void* scratch, int64_t scratch_bytes, void* stream,
                    const hbx_rules* rules);
/* hbx_kde_refit with `staged_host` in HOST memory (rows, then losses: n_new*(D+1) doubles; up to 256 staged
 * doubles of a budget of at most 1024 rows ride in the kernel arguments of the refit's first launch, no
 * host-to-device copy; more go through `scratch`), synchronous: when the call returns, `out_host` (host memory,
 * hbx_kde_refit_out_bytes) holds the output block.  The preparation's launches publish it to a device-mapped
 * host buffer, every 32-bit word as an 8-byte word flagged with the call's sequence number, and the call spins
 * until every word carries it (no copy launch, no blocking stream synchronisation).  The prepared models are
 * complete for work enqueued on `stream` afterwards; work on ANOTHER stream must first be ordered after the
 * refit (hbx_stream_order(other, stream)).  The drop-in's ObservationStore.refit calls this one
 * (bohb.py:211-251, one new_result per call). */
int hbx_kde_refit_sync(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype,
                       const double* staged_host, int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good,
                       double fac_bad, void* params_good, float* table_good, int64_t table_good_floats,
                       void* params_bad, float* table_bad, int64_t table_bad_floats, void* out, void* scratch,
                       int64_t scratch_bytes, void* stream, void* out_host);
/* hbx_kde_refit_sync under rules (as hbx_kde_refit_r; NULL: hbx_kde_refit_sync itself) */
int hbx_kde_refit_sync_r(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype,
                         const double* staged_host, int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good,
                         double fac_bad, void* params_good, float* table_good, int64_t table_good_floats,
                         void* params_bad, float* table_bad, int64_t table_bad_floats, void* out, void* scratch,
                         int64_t scratch_bytes, void* stream, void* out_host, const hbx_rules* rules);
/* Order stream `waiter` after all work enqueued on `signaller` so far (event record + stream wait, no host
 * wait): a model refit / prepared on one stream, used from another. */
int hbx_stream_order(void* waiter, void* signaller);

/* ---- KDE model preparation ----------------------------------------------------------------- */
/* Template bucket of the scoring kernel for dc continuous / du categorical dims
 * (stride = floats per 64-observation table chunk). */
int hbx_kde_bucket(int32_t dc, int32_t du, int32_t* dc_pad, int32_t* du_pad, int32_t* stride);
/* floats of the observation table of an n-row KDE in bucket (dc_pad, du_pad) */
int64_t hbx_kde_table_floats(int32_t n, int32_t dc_pad, int32_t du_pad);

/* Build one KDE for scoring.  X: device f64[*][D]; rows: device i64[n] (this KDE's rows, in
 * the reference's order); vartype/bw/nlev: host arrays of length D.  params: device buffer of
 * hbx_kde_param_bytes(); table: device f32[hbx_kde_table_floats(n, dc_pad, du_pad)].  info: host i32[8] =
 * {variant, nan_all, unsupported, dc, du, nconst, dc_pad, du_pad}.  variant selects the scoring kernel and is
 * passed back to hbx_kde_logpdf / hbx_kde_logpdf_rtol / hbx_kde_pair_bind; its bits:
 *   bit 0     has_neg: a categorical dim has a negative match factor (signed sums)
 *   bits 1-3  kc: 0 = categorical matching on the VALU; >= 1 = categorical one-hot product on the f16 matrix
 *             cores with kc K-steps
 *   bit 4     hmode: the whole exponent on the f16 matrix cores
 *   bit 5     exact_only: outside every fp32 scoring bucket (> 64 continuous / > 32 categorical dims), or a
 *             categorical dim with ONE observed level under a finite bandwidth h > 0 (match factor 1 - h, mismatch
 *             factor h / 0 = +inf: the pdf is finite, +inf or NaN): every candidate is evaluated in fp64
 *   bit 6     h32: the 32x32-tile kernels (with bit 4)
 *   bit 7     coarse: the table also holds the coarse layout of the acquisition's pre-screen instance
 *   bit 8     small_codes: <= 8 categorical slots, every code in [0, 3] (hbx_kde_logpdf_rtol's table look-up) */
int hbx_kde_prepare(const double* X, int32_t D, const int64_t* rows, int32_t n, const int32_t* vartype,
                    const double* bw, const int32_t* nlev, void* params, float* table, int64_t table_floats,
                    int32_t* info, void* stream);

/* ---- scoring ------------------------------------------------------------------------------- */
/* fp32 log-domain sums for Nc candidates (device f64[Nc][D]) against one prepared KDE;
 * est_out: device, Nc * hbx_kde_est_bytes() ({ln S+, ln S-, rel. bound, pad} per candidate). */
int hbx_kde_logpdf(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                   int32_t dc_pad, int32_t du_pad, int32_t variant, void* est_out, void* stream);

int64_t hbx_kde_workspace_bytes(int64_t Nc, int64_t nmax);

/* One acquisition: l = good KDE, g = bad KDE; selects the first index of the minimum of
 * max(f, g)/max(l, f) over the candidates (f: the pair's pdf_floor, hbx_kde_pair_set_rules; 1e-8 unless set),
 * exactly (fp64 re-score of every candidate whose
 * fp32 score interval reaches the minimum).  index_base is added to the reported index (GPU
 * sharding).  logl_out/logg_out: nullable device f32[Nc]: the fp32 ln pdf point estimates the
 * selection used (-inf for pdf <= 0, NaN for NaN).  Each lies within its own rigorous bound (what keeps
 * the selection exact), which is 1e-5 relative at D <= 32 away from outlying observations but NOT in
 * general (the fp32 expansion -|x'|^2 - |X'|^2 + 2 x'.X' cancels large terms next to outliers and beyond
 * D = 32); ln pdfs within the north-star 1e-5 everywhere come from hbx_kde_logpdf_rtol.  With both NULL
 * the scoring runs the fast instance (the
 * one-hot deltas' f16 lo parts moved into the bound: looser estimates, the same exact selection).  The
 * result record lives in the workspace: hbx_kde_result_ptr(workspace).
 * pair: the KDE pair's handle (hbx_kde_pair_bind, below; NULL: HBX_ERR_ARG).
 * events: NULL or hipEvent_t[3] (see hbx_event_create). */
int hbx_kde_acquire(const double* cand, int64_t Nc, int64_t index_base, const void* pair, float* logl_out,
                    float* logg_out, void* workspace, int64_t ws_bytes, void* events, void* stream);

/* A prepared (good, bad) KDE pair as every acquisition takes it -- hbx_kde_acquire, hbx_kde_acquire_bound,
 * hbx_kde_acquire_batch and hbx_kde_acquire_topk: its fixed arguments (D, each KDE's parameter block, table,
 * data, rows and variant as hbx_kde_prepare took / reported them, the shared bucket, nmax = the larger
 * observation count) are bound once.  The drop-in binds each model it fits (bohb.py:248-251 replaces the pair
 * on every refit), and a call passes only what changes -- about 2 us less host time per acquisition than
 * converting all of them.  The handle holds the pointers only: for all four calls the caller keeps the KDEs'
 * device buffers alive while it is in use, and frees it with hbx_kde_pair_free.  NULL on bad arguments
 * (hbx_last_error).
 * hbx_kde_acquire_bound: the synchronous acquisition (bohb.py:124-169 returns the pick to get_config's
 * caller): hbx_kde_acquire (fast scoring instances, no ln-pdf outputs) whose final kernel also
 * stores the 48-byte record into this thread's device-mapped host buffer, every 32-bit word as an 8-byte word
 * tagged with the call's sequence number; the call spins until every word carries its tag (bounded, then it
 * synchronises `stream`) and copies the record to rec_out (host, 48 bytes;
 * it also stays in the workspace, hbx_kde_result_ptr).  err (nullable, device u8[Nc], the GPU sampler's
 * domain-error flags): HBX_ACQ_DOMAIN_ERR is set in the record when any flag is set.  row_out (nullable, host
 * f64[D]): the winning candidate's row.  Both come with the record from the same final kernel: one wait for
 * the whole pick.  events: NULL or hipEvent_t[3] (hbx_kde_acquire). */
void* hbx_kde_pair_bind(int32_t D, const void* params_good, const float* table_good, const double* X_good,
                        const int64_t* rows_good, int32_t variant_good, const void* params_bad,
                        const float* table_bad, const double* X_bad, const int64_t* rows_bad, int32_t variant_bad,
                        int32_t dc_pad, int32_t du_pad, int64_t nmax);
/* The rules of every later acquisition on the handle (hbx_kde_acquire, _bound, _batch, _topk, staged or not): their
 * scores are formed with rules->pdf_floor.  A new handle has the reference snapshot's; NULL restores them.  Not to
 * be called while another thread runs an acquisition on the same handle. */
int hbx_kde_pair_set_rules(void* pair, const hbx_rules* rules);
int hbx_kde_acquire_bound(const void* pair, const double* cand, int64_t Nc, int64_t index_base, void* workspace,
                          int64_t ws_bytes, const uint8_t* err, void* events, void* stream, void* rec_out,
                          double* row_out);
void hbx_kde_pair_free(void* pair);

/* Batched acquisition: B = ceil(Nc / seg) independent get_config calls against the same model in one
 * pass (replaces B sequential runs of the bohb.py:124-169 loop, as an SH stage issues
 * them back to back, HB_iteration.py:136-138).  Candidates [b*seg, min((b+1)*seg, Nc)) belong to call b;
 * results: device buffer of B * hbx_acq_result_bytes() records, record b = call b's exact argmin with
 * the index relative to its segment start (+ index_base), -1 when the segment has no finite score.
 * Workspace: hbx_kde_batch_workspace_bytes(Nc, seg, nmax). */
int64_t hbx_kde_batch_workspace_bytes(int64_t Nc, int64_t seg, int64_t nmax);
int hbx_kde_acquire_batch(const double* cand, int64_t Nc, int64_t seg, int64_t index_base, const void* pair,
                          float* logl_out, float* logg_out, void* results, void* workspace, int64_t ws_bytes,
                          void* stream);

/* Top-k acquisition: the k best candidates of ONE pool, ranked exactly.  Where hbx_kde_acquire keeps the
 * first candidate of the smallest score (bohb.py:149-152: `if val < best`), this returns the first
 * min(k, F) entries of the stable ascending order of the score s = max(f, g)/max(l, f) (f: the pair's pdf_floor) over the F
 * candidates whose score is not NaN: ordered by (s[i], i), so equal scores come out in index order and entry 0
 * is hbx_kde_acquire's pick (index, score and both pdfs bit-identical).  The scoring launch and the exact fp64
 * re-score are hbx_kde_acquire's (fast scoring instances); the shortlist is taken against the k-th smallest
 * upper score bound instead of the smallest (csrc/hbx_topk.hip has the argument why it holds the whole top-k).
 * 1 <= k <= HBX_TOPK_MAX_K; k > Nc is legal (at most Nc entries come back).
 * results: device buffer of hbx_kde_topk_result_bytes(k) = 16 + 40 k bytes:
 *   header  {i32 count, i32 shortlist, i32 flags, i32 k}
 *           count: entries returned; shortlist: candidates re-scored in fp64; flags: HBX_ACQ_OVERFLOW (every
 *           rankable candidate re-scored), HBX_ACQ_NEAR_TIE (two adjacent returned entries, or the last
 *           returned one and the best re-scored one left out, lie within each other's error bounds `rel`)
 *   records count x {i64 index, f64 score, f64 pdf_l, f64 pdf_g, f32 rel, i32 0}   (40 bytes each, ranked)
 *           index: candidate index + index_base; score, pdf_l, pdf_g: the reference's fp64 values bit for
 *           bit; rel: the bound hbx_kde_acquire's record reports (hbx_kde_result_ptr)
 * Nc = 0: count = 0, nothing launched (the header zeroed).  Workspace: hbx_kde_topk_workspace_bytes(Nc, k,
 * nmax) (-1 for k out of range, as hbx_kde_topk_result_bytes).  Bad arguments: HBX_ERR_ARG (hbx_last_error).
 * Large calls on pairs the staged scoring serves (below, at hbx_kde_acquire_stats; the same HBX_STAGED switch, a
 * size threshold of its own, 4e9 candidates x observations) score g only for the candidates that can still rank: the seeds around the (k+1)-th largest l
 * and the candidates whose l-only bound f / max(l, f) does not exceed the seeds' (k+1)-th smallest upper
 * score bound.  count, flags and every record's index, score, pdf_l, pdf_g and rel are the unstaged call's,
 * exactly; the header's `shortlist` describes the screen and may differ (the evaluated candidates' fp32 estimates
 * come from launches with other observation splits).  The workspace begins with hbx_kde_acquire's, so
 * hbx_kde_acquire_stats(workspace, Nc, nmax) reports what the call did. */
#define HBX_TOPK_MAX_K 1024
int64_t hbx_kde_topk_workspace_bytes(int64_t Nc, int32_t k, int64_t nmax);
int64_t hbx_kde_topk_result_bytes(int32_t k);
int hbx_kde_acquire_topk(const double* cand, int64_t Nc, int32_t k, int64_t index_base, const void* pair,
                         void* results, void* workspace, int64_t ws_bytes, void* stream);

/* Grouped acquisition: ONE exact pick per KDE pair for B independent brackets -- what follows the batched refit
 * (hbx_seg_argsort_ex + hbx_kde_fit) when every bracket proposes a configuration (bohb.py:124-169 per bracket).
 * Every pointer is a device pointer.  X, seg_off, order, n_good, n_bad, vartype, bw_* and nlev_* are exactly
 * hbx_kde_fit's inputs and outputs, read where the fit left them: with n = seg_off[b+1] - seg_off[b], group b's
 * good KDE holds the rows X[seg_off[b] + order[seg_off[b] + j]], j < n_good[b], its bad KDE j in [n - n_bad[b], n).
 * cand: f64[B][C][D], group b's own pool.  results: B * hbx_acq_result_bytes() bytes, record b = what
 * hbx_kde_acquire returns for group b's pair over cand[b]: index (relative to the pool; -1: no finite score),
 * score, pdf_l and pdf_g the reference's fp64 values bit for bit; shortlist / near / rel / HBX_ACQ_OVERFLOW /
 * HBX_ACQ_NEAR_TIE with their meanings (hbx_kde_result_ptr) but from this path's own fp32 screen, so not the
 * single path's numbers; NEAR_TIE is set whenever two candidates share the best score.  Groups the fit skipped get
 * HBX_ACQ_NO_MODEL, groups with a categorical bandwidth / level count hbx_kde_prepare reports as unsupported get
 * HBX_ACQ_UNSUPPORTED: index -1, NaN score and pdfs -- never an error return.
 * Two launches on `stream`, no host synchronisation, no allocation, no per-group host work; B * C beyond int32:
 * HBX_ERR_ARG.  B == 0: nothing to do; C == 0: every record is the empty one (index -1, NaN score and pdfs).
 * workspace: hbx_kde_groups_workspace_bytes(B, C, D) bytes, 16-byte aligned (-1 for arguments out of range). */
#define HBX_ACQ_NO_MODEL    16  /* group skipped: n_good or n_bad is <= 0 or exceeds the segment (hbx_kde_fit's rule) */
#define HBX_ACQ_UNSUPPORTED 32  /* a categorical dim's bandwidth/levels are what hbx_kde_prepare reports as unsupported */
int64_t hbx_kde_groups_workspace_bytes(int64_t B, int64_t C, int32_t D);
int hbx_kde_acquire_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                           const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                           const double* bw_good, const double* bw_bad,
                           const int32_t* nlev_good, const int32_t* nlev_bad,
                           const double* cand, int64_t C, void* results,
                           void* workspace, int64_t ws_bytes, void* stream);
/* The same for S get_config requests per bracket in one call: a successive-halving stage issues num_configs[stage]
 * get_config calls back to back against one model (HB_iteration.py:136-138), each with its own num_samples
 * candidates and its own strict-'<' argmin (bohb.py:124-169).  The model arguments are hbx_kde_acquire_groups',
 * unchanged.  cand: f64[B][S][C][D], request (b, s)'s own pool of C candidates.  results: B * S records, record
 * b * S + s = what hbx_kde_acquire_groups returns for group b over cand[b][s]: index (relative to the request's
 * pool), score, pdf_l and pdf_g the reference's fp64 values bit for bit; HBX_ACQ_NO_MODEL / HBX_ACQ_UNSUPPORTED as
 * there.  Requests never see one another: the bound, the shortlist, the first-certain-1 rule, the argmin and the
 * near count are per request.  shortlist / near / rel / HBX_ACQ_OVERFLOW / HBX_ACQ_NEAR_TIE keep their meanings but
 * may come from another fp32 screen than the one-request call's (a group's S * C candidates are screened as one
 * flattened pool, by a kernel chosen from its size) -- except with S == 1, which runs hbx_kde_acquire_groups' own
 * two launches: the B records are byte-identical.  Two launches on `stream`, no host synchronisation, no
 * allocation, no per-group host work, never an error return for a bad group; B * S * C beyond int32: HBX_ERR_ARG
 * (the size helper: -1).  B == 0 or S == 0: nothing to do; C == 0: B * S empty records.  workspace:
 * hbx_kde_groups_batch_workspace_bytes(B, S, C, D) bytes, 16-byte aligned.
 * Candidates: hbx_kde_sample_groups with pool size S * C -- candidate (b, s, i) then draws from the Philox counter
 * counter_base + (b * S + s) * C + i. */
int64_t hbx_kde_groups_batch_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D);
int hbx_kde_acquire_groups_batch(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                 const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                 const double* bw_good, const double* bw_bad,
                                 const int32_t* nlev_good, const int32_t* nlev_bad,
                                 const double* cand, int64_t S, int64_t C, void* results,
                                 void* workspace, int64_t ws_bytes, void* stream);
/* hbx_kde_acquire_groups_batch with the scores formed under rules->pdf_floor (NULL: the same call); S = 1 is
 * hbx_kde_acquire_groups under those rules. */
int hbx_kde_acquire_groups_batch_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                   const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                   const double* bw_good, const double* bw_bad,
                                   const int32_t* nlev_good, const int32_t* nlev_bad,
                                   const double* cand, int64_t S, int64_t C, void* results,
                                   void* workspace, int64_t ws_bytes, void* stream, const hbx_rules* rules);
/* Grouped top-k: the k best candidates of every bracket's own pool in one call -- hbx_kde_acquire_topk's answer for
 * each of hbx_kde_acquire_groups' B groups.  The model arguments are hbx_kde_acquire_groups', unchanged; cand:
 * f64[B][C][D]; 1 <= k <= HBX_TOPK_MAX_K, k > C is legal.  results: B blocks of hbx_kde_topk_result_bytes(k) =
 * 16 + 40 k bytes, block b at b * hbx_kde_topk_result_bytes(k), each with hbx_kde_acquire_topk's layout: header
 * {i32 count, i32 shortlist, i32 flags, i32 k}, then `count` ranked records {i64 index, f64 score, f64 pdf_l,
 * f64 pdf_g, f32 rel, i32 0}; the bytes of a block past its `count` records are unspecified.  Block b holds the first
 * min(k, F) entries of the ascending order by (score, index) over the F candidates of cand[b] whose score is not NaN:
 * index relative to the pool, score and both pdfs the reference's fp64 values bit for bit, entry 0 =
 * hbx_kde_acquire_groups' record for the group (index, score, pdfs).  count = 0 when no score is rankable; groups
 * without a model / with an unsupported dim: count = 0 and HBX_ACQ_NO_MODEL / HBX_ACQ_UNSUPPORTED in flags, never an
 * error return.  HBX_ACQ_OVERFLOW: every candidate of the group was re-scored.  HBX_ACQ_NEAR_TIE: two adjacent
 * returned entries, or the last returned one and the best re-scored one left out, lie within each other's `rel` --
 * or the last returned entry scores exactly 1 and candidates whose score is certainly exactly 1 were not listed
 * (only the first k of them by index are re-scored: csrc/hbx_groups.hip has the argument).
 * Two launches on `stream` (hbx_kde_acquire_groups' screen, then one select block per group), no host
 * synchronisation, no allocation, no per-group host work.  B == 0: nothing to do; C == 0: B headers {0, 0, 0, k}.
 * B * C beyond int32, k out of range, null pointers, misalignment (workspace 16, results 8 bytes) or a short
 * workspace: HBX_ERR_ARG (hbx_last_error).  workspace: hbx_kde_groups_topk_workspace_bytes(B, C, k, D) bytes (the
 * grouped call's plus 16 bytes per candidate for the re-scored pdfs; -1 for arguments out of range). */
int64_t hbx_kde_groups_topk_workspace_bytes(int64_t B, int64_t C, int32_t k, int32_t D);
int hbx_kde_acquire_groups_topk(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                const double* bw_good, const double* bw_bad,
                                const int32_t* nlev_good, const int32_t* nlev_bad,
                                const double* cand, int64_t C, int32_t k, void* results,
                                void* workspace, int64_t ws_bytes, void* stream);
/* hbx_kde_acquire_groups_topk with the scores formed under rules->pdf_floor (NULL: the same call) */
int hbx_kde_acquire_groups_topk_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                  const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                  const double* bw_good, const double* bw_bad,
                                  const int32_t* nlev_good, const int32_t* nlev_bad,
                                  const double* cand, int64_t C, int32_t k, void* results,
                                  void* workspace, int64_t ws_bytes, void* stream, const hbx_rules* rules);
/* Grouped ln-pdf: ln l(x) and ln g(x) for every candidate of every bracket's pool in one call -- hbx_kde_logpdf_rtol's
 * contract for each of hbx_kde_acquire_groups' B groups.  The model arguments are hbx_kde_acquire_groups', unchanged,
 * read where hbx_kde_fit left them (no KdeParams, no table, no prepare); cand: f64[B][C][D] (S requests per group:
 * the flattened pool, C := S * C).  ln_l, ln_g: f64[B][C], either may be NULL (that KDE is skipped; both NULL is
 * HBX_ERR_ARG).  Every value is ln pdf within rtol * max(1, |ln p|) of the reference's KDEMultivariate.pdf, -inf
 * where the pdf is 0, NaN where the reference's pdf is NaN or negative.  status: i32[B]: HBX_ACQ_NO_MODEL /
 * HBX_ACQ_UNSUPPORTED by hbx_kde_acquire_groups' rules -- all of that group's outputs are NaN, never an error return
 * -- and HBX_GRP_EXACT_L / HBX_GRP_EXACT_G where that KDE's values are ln of the bit-exact fp64 pdf (a negative
 * categorical match factor h > 1, a single observed level, a continuous bandwidth that is not positive and finite,
 * dims beyond the slot bucket): NaN where that pdf is negative or NaN, -inf where it underflows to 0.
 * flags: HBX_LOGPDF_FP64_ONLY skips the fp32 first pass (the fp64 pass alone meets the contract; the fp32 pass only
 * writes values its own rigorous bound certifies).  rtol > 0; below 1e-5 the fp64 pass uses fp64 exponentials.
 * Launches on `stream` only: no host synchronisation, no allocation, no per-group host work.  B == 0 or C == 0:
 * nothing to do (status is not written).  B * C beyond int32, D outside [1, hbx_max_dims()], null or misaligned
 * pointers (f64 / i64: 8 bytes, i32: 4, workspace: 16) or a short workspace: HBX_ERR_ARG (hbx_last_error), before the
 * first launch.  workspace: hbx_kde_logpdf_groups_workspace_bytes(B, C, D) bytes (-1 for arguments out of range); its
 * header holds four counters of output values, read by hbx_kde_logpdf_groups_stats (synchronises the device):
 * out4[0] written by the fp32 pass, [1] by the fp64 log-space pass, [2] through the exact pdf, [3] NaN-filled for
 * groups without a usable model; their sum is B * C times the number of non-NULL outputs. */
#define HBX_GRP_EXACT_L 64
#define HBX_GRP_EXACT_G 128
#define HBX_LOGPDF_FP64_ONLY 1
int64_t hbx_kde_logpdf_groups_workspace_bytes(int64_t B, int64_t C, int32_t D);
int hbx_kde_logpdf_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                          const double* bw_good, const double* bw_bad,
                          const int32_t* nlev_good, const int32_t* nlev_bad,
                          const double* cand, int64_t C, double rtol, int32_t flags,
                          double* ln_l, double* ln_g, int32_t* status,
                          void* workspace, int64_t ws_bytes, void* stream);
int hbx_kde_logpdf_groups_stats(const void* workspace, int64_t* out4);
/* The matching sampler: C candidates per group around its good KDE's rows (hbx_kde_sample's rule).  Candidate
 * (b, i) is byte-equal to what hbx_kde_sample draws for group b's good KDE (tab = NULL) at candidate index i of a
 * call with counter_base + b * C.  cands: f64[B][C][D] (16-byte aligned when D is even); domain_err: nullable
 * u8[B][C].  Groups without a model (n_good[b] <= 0 or past the segment): NaN rows, flags 0.  One launch, no host
 * synchronisation. */
int hbx_kde_sample_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const double* bw_good, const int32_t* levels,
                          double bw_factor, uint64_t seed, uint64_t counter_base, uint32_t stream_id,
                          int64_t C, double* cands, uint8_t* domain_err, void* stream);
/* Grouped get_config, the finish step: the configuration vector of every one of B x S requests after a grouped
 * acquisition (bohb.py:107-111,154-166).  Request q = b * S + s has its record records[q]
 * (hbx_kde_acquire_groups_batch's layout; S = 1: hbx_kde_acquire_groups'), its pool cands[q][C][D] and its sampler
 * flags domain_err[q][C].  source_out[q], by the first rule that matches, and rows_out[q][0..D):
 *   2 HBX_CFG_NO_MODEL         the record's flags carry HBX_ACQ_NO_MODEL or HBX_ACQ_UNSUPPORTED, or records == NULL
 *                              (bohb.py:109: no model for the run)                                       prior draw
 *   1 HBX_CFG_RANDOM_FRACTION  u_q < random_fraction (bohb.py:109)                                       prior draw
 *   4 HBX_CFG_DOMAIN_ERR       a byte of domain_err[q][0..C) is not zero (bohb.py:163-166: the sampler raised)
 *                                                                                                        prior draw
 *   3 HBX_CFG_NO_SCORE         the record's index < 0 (bohb.py:154-157: best_vector is None)             prior draw
 *   0 HBX_CFG_MODEL            otherwise                                       cands[q][index][:], copied bit for bit
 * The request's draws use its first candidate counter ctr_q = counter_base + q * C with hbx_kde_sample_groups' seed
 * and stream_id and counter words the sampler never uses, so they never meet a candidate's draws and do not depend on
 * the other groups of the call: u_q = u01(bits64(philox(ctr_q, 0xFFFFFFFE), 0)); the prior of dims 2p and 2p + 1
 * from philox(ctr_q, 0xFFFE0000 + p), u = u01(bits64(r, 0)) and u01(bits64(r, 1)) (u01: ((bits >> 11) + 0.5) 2^-53,
 * open): levels[d] == 0 gives u (configspace.py:62), levels[d] = t > 0 gives (double)min(t - 1, floor(t u))
 * (configspace.py:97,113).  numpy's interval is half-open, this one open: parity with the reference's prior is
 * distributional, as for the sampler.
 * records may be NULL (every request HBX_CFG_NO_MODEL; cands and domain_err are then not read); domain_err may be NULL
 * (no HBX_CFG_DOMAIN_ERR).  C >= 1.  An index not below C, which no acquisition writes, is treated as HBX_CFG_NO_SCORE
 * and never used as an offset.  rows_out: f64[B][S][D]; source_out: u8[B][S].  One launch on `stream`, no host
 * synchronisation; the records are not written.  B == 0 or S == 0: nothing to do.  Null pointers, B * S * C beyond
 * int32, D outside [1, hbx_max_dims()], random_fraction outside [0, 1] or NaN: HBX_ERR_ARG. */
#define HBX_CFG_MODEL 0
#define HBX_CFG_RANDOM_FRACTION 1
#define HBX_CFG_NO_MODEL 2
#define HBX_CFG_NO_SCORE 3
#define HBX_CFG_DOMAIN_ERR 4
int hbx_kde_finish_groups(const void* records, const double* cands, const uint8_t* domain_err, const int32_t* levels,
                          int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                          uint64_t counter_base, uint32_t stream_id, double* rows_out, uint8_t* source_out, void* stream);
/* Grouped get_config whole (bohb.py:104-169 for S requests of each of B brackets): hbx_kde_sample_groups (pool S * C
 * per group) + hbx_kde_acquire_groups_batch + hbx_kde_finish_groups with the same seed, counter_base and stream_id,
 * on one stream, no host synchronisation -- by definition that composition, byte for byte.  The model arguments are
 * hbx_kde_acquire_groups_batch's.  The pools and error bytes live in the workspace (hbx_kde_propose_groups_ws_offsets:
 * byte offsets of [pools f64[B][S][C][D], error bytes u8[B][S][C], records, end]); records_out (B * S records,
 * 8-byte aligned) and cands_out (f64[B][S][C][D]) -- either may be NULL -- receive the records and a copy of the
 * pools.  Requests that end up random are still sampled and scored.  workspace:
 * hbx_kde_propose_groups_workspace_bytes(B, S, C, D) bytes, 16-byte aligned (-1 for arguments out of range, C < 1
 * included).  Argument errors as hbx_kde_finish_groups', plus a short or misaligned workspace. */
int64_t hbx_kde_propose_groups_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D);
int hbx_kde_propose_groups_ws_offsets(int64_t B, int64_t S, int64_t C, int32_t D, int64_t* out4);
int hbx_kde_propose_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                           const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                           const double* bw_good, const double* bw_bad,
                           const int32_t* nlev_good, const int32_t* nlev_bad, const int32_t* levels,
                           double bandwidth_factor, double random_fraction, uint64_t seed, uint64_t counter_base,
                           uint32_t stream_id, int64_t S, int64_t C, double* rows_out, uint8_t* source_out,
                           void* records_out, double* cands_out, void* workspace, int64_t workspace_bytes, void* stream);
/* hbx_kde_propose_groups with hbx_kde_acquire_groups_batch_r in the middle of the composition (NULL: the same call) */
int hbx_kde_propose_groups_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                             const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                             const double* bw_good, const double* bw_bad,
                             const int32_t* nlev_good, const int32_t* nlev_bad, const int32_t* levels,
                             double bandwidth_factor, double random_fraction, uint64_t seed, uint64_t counter_base,
                             uint32_t stream_id, int64_t S, int64_t C, double* rows_out, uint8_t* source_out,
                             void* records_out, double* cands_out, void* workspace, int64_t workspace_bytes, void* stream,
                             const hbx_rules* rules);
/* The request mask: the four grouped get_config calls with only the wanted requests computed.  want: device
 * u8[B][S], request (b, s) is wanted when its byte is not zero; want == NULL: every request is wanted.  The Philox
 * counter of request q = b * S + s is fixed by its position (counter_base + q * C + i), so: EVERY WANTED REQUEST GETS
 * EXACTLY THE BYTES THE DENSE CALL GIVES IT, AND AN UNWANTED REQUEST COSTS NOTHING AND IS MARKED AS SKIPPED.  The
 * grids are the dense calls'; the host never reads the mask and nothing synchronises -- blocks and waves test it.
 * The model arguments are the dense calls', unchanged; so are the argument checks (before the first launch).
 *
 * hbx_kde_sample_groups_m: candidate (b, s, i) of a wanted request is byte-equal to hbx_kde_sample_groups' draw for
 *   it with pool size S * C.  The rows and error bytes of an unwanted request are not written (the error bytes are
 *   zeroed first, all of them, as there).
 * hbx_kde_acquire_groups_batch_m: a wanted request's record is hbx_kde_acquire_groups_batch(_r)'s, all 48 bytes (the
 *   screen is chosen from S and the dense tile count, and a candidate's sums do not depend on the other candidates).
 *   An unwanted request gets the empty record -- index -1, NaN score and pdfs, shortlist and near 0 -- with
 *   HBX_ACQ_SKIPPED and the group's HBX_ACQ_NO_MODEL / HBX_ACQ_UNSUPPORTED bit as the dense call sets it.  rules may be
 *   NULL.  The workspace (hbx_kde_groups_batch_workspace_bytes) starts with four counters that
 *   hbx_kde_groups_request_stats reads (it synchronises the device): out4[0] requests answered, [1] requests skipped,
 *   [2] candidates the screen evaluated, [3] candidates re-scored in fp64.  C == 0: empty records (skipped ones for
 *   unwanted requests), no counters.
 * hbx_kde_finish_groups_m: a rule ahead of hbx_kde_finish_groups' five -- an unwanted request gets
 *   source_out[q] = HBX_CFG_SKIPPED and a NaN row; wanted requests go by the five rules.
 * hbx_kde_random_requests_groups: want_out[q] = (want_in == NULL or want_in[q] != 0) and not (u_q < random_fraction),
 *   u_q the finish step's draw -- the requests that a model has to answer.  One launch.
 * hbx_kde_propose_groups_m: the composition of the three on one stream.  flags & HBX_PROPOSE_SKIP_RANDOM: the sampler
 *   and the acquisition run under hbx_kde_random_requests_groups' mask (kept in the workspace), the finish step under
 *   want.  Rule 1 (HBX_CFG_RANDOM_FRACTION) comes before the rules that read the pool, so rows_out and source_out are
 *   byte-equal to the call without the flag; a random request has a skipped record and its pool is not written.
 *   Without the flag, requests that end up random are still sampled and scored.  cands_out, when given (16-byte
 *   aligned), IS the pool: unwanted requests' rows stay as they were.  workspace:
 *   hbx_kde_propose_groups_m_workspace_bytes bytes; hbx_kde_propose_groups_m_ws_offsets: byte offsets of [pools, error
 *   bytes, records, mask, end]. */
#define HBX_ACQ_SKIPPED 64  /* the record of a request the mask left out (the next free bit of the record's flags) */
#define HBX_CFG_SKIPPED 5
#define HBX_PROPOSE_SKIP_RANDOM 1
int hbx_kde_sample_groups_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                            const int64_t* n_good, const double* bw_good, const int32_t* levels,
                            double bw_factor, uint64_t seed, uint64_t counter_base, uint32_t stream_id,
                            int64_t S, int64_t C, const uint8_t* want, double* cands, uint8_t* domain_err, void* stream);
int hbx_kde_acquire_groups_batch_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                   const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                   const double* bw_good, const double* bw_bad,
                                   const int32_t* nlev_good, const int32_t* nlev_bad,
                                   const double* cand, int64_t S, int64_t C, const uint8_t* want, void* results,
                                   void* workspace, int64_t ws_bytes, void* stream, const hbx_rules* rules);
int hbx_kde_groups_request_stats(const void* workspace, int64_t* out4);
int hbx_kde_finish_groups_m(const void* records, const double* cands, const uint8_t* domain_err, const int32_t* levels,
                            int32_t D, int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                            uint64_t counter_base, uint32_t stream_id, const uint8_t* want, double* rows_out,
                            uint8_t* source_out, void* stream);
int hbx_kde_random_requests_groups(int64_t B, int64_t S, int64_t C, double random_fraction, uint64_t seed,
                                   uint64_t counter_base, uint32_t stream_id, const uint8_t* want_in, uint8_t* want_out,
                                   void* stream);
int64_t hbx_kde_propose_groups_m_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D);
int hbx_kde_propose_groups_m_ws_offsets(int64_t B, int64_t S, int64_t C, int32_t D, int64_t* out5);
int hbx_kde_propose_groups_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                             const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                             const double* bw_good, const double* bw_bad,
                             const int32_t* nlev_good, const int32_t* nlev_bad, const int32_t* levels,
                             double bandwidth_factor, double random_fraction, uint64_t seed, uint64_t counter_base,
                             uint32_t stream_id, int64_t S, int64_t C, const uint8_t* want, int32_t flags,
                             double* rows_out, uint8_t* source_out, void* records_out, double* cands_out,
                             void* workspace, int64_t workspace_bytes, void* stream, const hbx_rules* rules);

/* ---- conditional search spaces ---------------------------------------------------------------
 * An observation of a conditional space holds NaN where a hyperparameter is inactive.  Released hpbandster imputes
 * such entries before the KDEs are fitted (impute_conditional_data, a rule added after the reference snapshot);
 * hbx_kde_impute_groups is that rule for B groups, with Philox draws instead of numpy's global stream and with every
 * NaN filled (a NaN in dim 0 alone included).
 *
 * The good and the bad set of a group are imputed independently, each from its own ORIGINAL rows.  A set is the ns
 * rows j = 0 .. ns - 1 in split order (hbx_kde_fit's convention: good order[seg_off[b] + j], j < n_good[b]; bad
 * order[seg_off[b+1] - n_bad[b] + j], j < n_bad[b]).  A row of the set is copied to its view row v; then, for
 * t = 0, 1, ... while it holds a NaN, with d0 its lowest NaN dim and m the set rows whose original value at d0 is
 * not NaN (+-inf is a value):
 *   m > 0    the donor is the k-th such row in ascending j, k = min(m - 1, floor(u_a m)); EVERY NaN dim of the row
 *            takes the donor's original value, which may be NaN again
 *   m == 0   dim d0 takes the prior: u_b where levels[d0] == 0, else (double)min(L - 1, floor(L u_b)), L = levels[d0]
 * r = philox(counter_base + v, 0xFFFD0000 + t) under seed / stream_id as in hbx_kde_sample_groups,
 * u_a = u01(bits64(r, 0)), u_b = u01(bits64(r, 1)).  At most D iterations per row.
 *
 * The view.  view_off: device i64[B+1], given by the caller: view_off[b+1] - view_off[b] is n_good[b] + n_bad[b]
 * for a group hbx_kde_fit would model and 0 for a skipped one.  Group b's view rows are its imputed good rows, then
 * its imputed bad rows (a row in both sets occurs twice, imputed separately).  Xv: f64[Nv][D]; order_v: i64[Nv], the
 * identity local positions; src_v: i32[Nv], the original local row of each view row; counts: nullable i32[B][2],
 * entries filled from donors / from the prior.  (Xv, view_off, order_v, n_good, n_bad) is then a model for every
 * grouped entry point as it is: head n_good rows and tail n_bad rows of a segment of n_good + n_bad.  Rows without
 * NaN are byte copies.  A group whose view length does not match its sizes (or leaves [0, Nv]) is left unwritten,
 * counts -1 -- not an error return.  X, D, seg_off, B, order, n_good, n_bad: hbx_kde_fit's; levels: i32[D].
 * Stream-ordered, no allocation, no host synchronisation.  workspace: hbx_kde_impute_groups_workspace_bytes(Nv, B, D)
 * bytes, 16-byte aligned (-1 for arguments out of range); the per-dim masks of a set live in LDS where they fit and
 * there otherwise (environment HBX_IMPUTE_LDS=0: always there).  Null or misaligned pointers, D outside
 * [1, hbx_max_dims()], negative sizes, a short workspace: HBX_ERR_ARG before any launch.  B == 0 or Nv == 0: nothing
 * to do.  hbx_kde_impute_groups_host: the same rule in plain loops over host memory, byte for byte. */
int64_t hbx_kde_impute_groups_workspace_bytes(int64_t Nv, int64_t B, int32_t D);
int hbx_kde_impute_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                          const int64_t* n_good, const int64_t* n_bad, const int32_t* levels, const int64_t* view_off,
                          int64_t Nv, uint64_t seed, uint64_t counter_base, uint32_t stream_id, double* Xv,
                          int64_t* order_v, int32_t* src_v, int32_t* counts, void* workspace, int64_t ws_bytes,
                          void* stream);
int hbx_kde_impute_groups_host(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                               const int64_t* n_good, const int64_t* n_bad, const int32_t* levels,
                               const int64_t* view_off, int64_t Nv, uint64_t seed, uint64_t counter_base,
                               uint32_t stream_id, double* Xv, int64_t* order_v, int32_t* src_v, int32_t* counts);
/* Deactivate the inactive dims of N rows in place (what makes a proposed vector a valid configuration of a
 * conditional space; ConfigSpace's deactivate_inactive_hyperparameters).  Conditions i = 0 .. n_cond - 1, in
 * topological order: rows[r][child[i]] becomes NaN when rows[r][parent[i]] is NaN or is not an integer level in
 * [0, 64) whose bit is set in allowed[i].  child / parent: device i32[n_cond]; allowed: device u64[n_cond].  One
 * thread per row, one launch on `stream`.  hbx_rows_deactivate_host: the same over host memory. */
int hbx_rows_deactivate(double* rows, int64_t N, int32_t D, const int32_t* child, const int32_t* parent,
                        const uint64_t* allowed, int64_t n_cond, void* stream);
int hbx_rows_deactivate_host(double* rows, int64_t N, int32_t D, const int32_t* child, const int32_t* parent,
                             const uint64_t* allowed, int64_t n_cond);

/* Optional timing: `events` of hbx_kde_acquire is NULL or an array of three hipEvent_t recorded on
 * `stream` before the l scoring launch, between l and g, and after g -- or, when l and g are scored by
 * one pair launch (both KDEs on the same hmode kernel, HBX_SCORE_PAIR not 0), only [0] before and [1]
 * after it. */
int hbx_event_create(void** ev);
int hbx_event_destroy(void* ev);
int hbx_event_elapsed_ms(void* start, void* stop, float* ms);

/* Copy `bytes` of device memory (e.g. the result record) to host memory on `stream` and wait for it without
 * a blocking synchronisation: up to 4096 bytes go through the calling thread's device-mapped host buffer
 * (allocated on the thread's first call and kept for its lifetime, ~8.4 KB with hbx_kde_acquire_bound's
 * tagged region; when the thread ends it goes back to a process-wide pool for the next thread) with a
 * completion word the
 * call spins on; larger or unaligned copies poll the stream.  Replaces the caller's copy + synchronise
 * after hbx_kde_acquire (the reference's get_config returns the pick to its caller: bohb.py:166). */
int hbx_fetch(void* host_dst, const void* dev_src, int64_t bytes, void* stream);

/* Device-mapped host buffers this process has allocated (hbx_fetch / hbx_kde_acquire_bound's and the refits'):
 * bounded by the threads calling at once, not by the threads that ever called -- a thread's buffer is pooled
 * when the thread ends.  Diagnostic (tests). */
int64_t hbx_mapped_host_buffers(void);

/* Device address of the result record inside an acquisition workspace (48 bytes):
 *   {i64 index, f64 score, f32 rel, i32 flags, i32 shortlist, i32 near, f64 pdf_l, f64 pdf_g}
 * index: first index of the minimal exact score (-1: no finite score); rel: bound of
 * |score - the same score in numpy's arithmetic| / score; near: candidates whose scores lie within those
 * bounds of the winner's (itself included).  flags: HBX_ACQ_OVERFLOW (1: every candidate re-scored),
 * HBX_ACQ_NEAR_TIE (2: near > 1 -- the fp64 re-score here and numpy may order them differently, so the
 * near set (hbx_kde_ws_offsets) must be re-scored in the reference's own arithmetic to pick the
 * reference's index; the Python wrapper does this on the host and sets HBX_ACQ_RESOLVED, 4). */
#define HBX_ACQ_OVERFLOW 1
#define HBX_ACQ_NEAR_TIE 2
#define HBX_ACQ_RESOLVED 4
#define HBX_ACQ_DOMAIN_ERR 8  /* hbx_kde_acquire_bound with err: a candidate's draw hit a domain error */
void* hbx_kde_result_ptr(void* workspace);
/* Byte offsets of [shortlist count (i32), shortlist (i32 candidate indices), near list, exact l (f64),
 * exact g (f64)] inside the workspace of an acquisition over (Nc, seg, nmax) candidates (seg = Nc for
 * hbx_kde_acquire).  hbx_kde_acquire's near list holds the near set's candidate indices (record.near of
 * them); hbx_kde_acquire_batch's holds a 0/1 flag per shortlist entry. */
int hbx_kde_ws_offsets(int64_t Nc, int64_t seg, int64_t nmax, int64_t* out);
/* Staged scoring of hbx_kde_acquire / hbx_kde_acquire_bound without ln-pdf outputs (both KDEs on the coarse
 * 32x32 instance, Nc * nmax large enough; environment HBX_STAGED=0: never, 2: wherever supported): l is scored for
 * every candidate, g only for the candidates l alone does not rule out (score >= f / max(l, f) whatever g
 * is).  The pick (index, score, pdf_l, pdf_g, and with them near and rel) is the unstaged call's, exactly.  The
 * screen's own figures can differ: `shortlist` is normally equal or lower by one (the first certain f/f tie,
 * when it was pruned and cannot win); the evaluated candidates' fp32 estimates come from launches with their own
 * observation splits -- valid bounds, not the fused launch's bits -- so a candidate at the very edge of the
 * shortlist can fall on either side; a pruned candidate whose coarse g bound alone would pass the overflow limit
 * sets HBX_ACQ_OVERFLOW (and the whole-set re-score) in the unstaged call only; and when l itself sets
 * HBX_ACQ_OVERFLOW the staged shortlist also holds the pruned certain ties, so it can be longer.
 * hbx_kde_acquire_stats: what the last single acquisition or top-k call (hbx_kde_acquire_topk) on `workspace`
 * (sized for Nc, nmax) did -- a device read, synchronising: out[0] = 1 when it staged, [1] seeds, [2] survivors,
 * [3] candidates whose g was evaluated (Nc when it did not stage).  Every such call leaves these words valid: an
 * unstaged call on a workspace an earlier staged call used reports 0. */
int hbx_kde_acquire_stats(const void* workspace, int64_t Nc, int64_t nmax, int64_t* out);
/* Stage 1 of the last staged single acquisition on `workspace` (a device read, synchronising): out[0] = 1 when
 * every candidate's l bound and the largest lower l bound came from the good KDE's scoring launch itself (its
 * unsplit form; environment HBX_STAGE1_LHI=0: never), 0 when a launch of their own derived them or the call did
 * not stage; out[1] = that largest lower bound as the workspace keeps it, an order-preserving uint32 of the float. */
int hbx_kde_acquire_stage1(const void* workspace, int64_t Nc, int64_t nmax, int64_t* out);

int64_t hbx_kde_pdf_scratch_bytes(int64_t nmax);

/* Exact fp64 pdf of one prepared KDE at Np points (device f64[Np][D]) -> out (device f64[Np]).  Same
 * float64 operations in the same order as statsmodels 0.12.2 on the pinned numpy 1.26.4 (its SVML exp
 * restated bit for bit, numpy's pairwise sums): bit-identical to the reference's KDEMultivariate.pdf.
 * Np = 0: nothing to do (pts / out may be NULL); likewise hbx_kde_logpdf_exact. */
int hbx_kde_pdf_exact(const double* pts, int64_t Np, int32_t D, const void* params, const double* X,
                      const int64_t* rows, int64_t n, double* out, void* scratch, int64_t scratch_bytes,
                      void* stream);
/* ln KDEMultivariate.pdf (SM:kernel_density.py:162-196) in fp64 log space: logsumexp over the
 * observations of the log kernel products (no fp64 underflow, ~1e-15 relative).  NaN for KDEs with
 * negative categorical factors or structural NaNs -- use hbx_kde_pdf_exact there.  out: device f64[Np]. */
int hbx_kde_logpdf_exact(const double* pts, int64_t Np, int32_t D, const void* params, const double* X,
                         const int64_t* rows, double* out, void* stream);

/* ln pdf of one prepared KDE at Nc candidates within rtol * max(1, |ln pdf|) of the reference's
 * KDEMultivariate.pdf (kernel_density.py:162-196) -- the north-star contract at every D: the fp32
 * estimate (hbx_kde_logpdf) wherever its rigorous per-candidate bound guarantees rtol, the fp64 log-space
 * evaluation (hbx_kde_logpdf_exact) for the rest -- candidates next to outlying observations, beyond
 * D = 32, exact-only KDEs -- and ln of the exact fp64 pdf for KDEs with negative categorical factors.
 * All on the device.  cand: device f64[Nc][D]; X / rows: the KDE's observations (as hbx_kde_pdf_exact);
 * out: device f64[Nc] (-inf: pdf 0; NaN where the reference's pdf is NaN or negative);
 * scratch: hbx_kde_logpdf_rtol_scratch_bytes(Nc) device bytes. */
int64_t hbx_kde_logpdf_rtol_scratch_bytes(int64_t Nc);
int hbx_kde_logpdf_rtol(const double* cand, int64_t Nc, int32_t D, const void* params, const float* table,
                        const double* X, const int64_t* rows, int32_t dc_pad, int32_t du_pad, int32_t variant,
                        double rtol, double* out, void* scratch, int64_t scratch_bytes, void* stream);

/* numpy 1.26.4's float64 exp (what the reference's np.exp computes on AVX512_SKX hosts), element-wise
 * on the device: the known-answer check of the exact re-score's exp.  x, y: device f64[n]. */
int hbx_np_exp(const double* x, int64_t n, double* y, void* stream);

/* ---- candidate sampler (bohb.py:133-147, on the GPU) --------------------------------------- */
/* Philox4x32-10 block function (host): out[4] = philox(counter[4], key[2]).  Exposed for the
 * known-answer tests of the generator the sampler uses. */
int hbx_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* Nc candidates around the good KDE's observations, BOHB's rule: datum = rows[U{0..n-1}], then per
 * dim truncnorm(-m/bw, (1-m)/bw, loc=m, scale=bw_factor*bw) (levels[d] == 0) or keep-with-prob-(1-bw)
 * / U{0..t-1} (levels[d] = t).  X: device f64[*][D]; rows: device i64[n] (the good KDE's rows);
 * bw: device f64[D]; levels: device i32[D].  Dims 2k, 2k+1 of candidate i use Philox counter
 * (counter_base + i, k, stream_id) under key = seed (32-bit words: the uniform, the categorical level
 * draw), so consecutive calls with advancing counter_base equal one call over the union; the truncnorm
 * inversion is fp32 on the smaller tail (distributional parity).  cands: device f64[Nc][D], 16-byte
 * aligned when D is even; datum: nullable device i64[Nc] (drawn row positions);
 * domain_err: nullable device u8[Nc], 1 where a continuous dim's bounds fail scipy's a < b check
 * (the reference's call raises and falls back to a random configuration). */
int hbx_kde_sample(const double* X, int32_t D, const int64_t* rows, int64_t n, const double* bw,
                   const int32_t* levels, const double* tab, double bw_factor, uint64_t seed, uint64_t counter_base,
                   uint32_t stream_id, int64_t Nc, double* cands, int64_t* datum, uint8_t* domain_err, void* stream);
/* Standard normal quantile Phi^-1 (device f64[n] -> device f64[n]) in fp64 (Wichura's AS 241,
 * scipy.special.ndtri semantics on (0, 1)). */
int hbx_norm_ppf(const double* p, int64_t n, double* z, void* stream);
/* Optional per-model table for hbx_kde_sample (`tab`, nullable): Phi at the standardised truncnorm
 * bounds of every (good row, continuous dim), device f64[hbx_kde_sample_table_bytes(n, D) / 8].  Same
 * draws with or without it; it saves two normcdf per draw when Nc >> n. */
int64_t hbx_kde_sample_table_bytes(int64_t n, int32_t D);
int hbx_kde_sample_table(const double* X, int32_t D, const int64_t* rows, int64_t n, const double* bw,
                         const int32_t* levels, double* tab, void* stream);

/* ---- cross-validation bandwidth objectives (KDEMultivariate bw='cv_ls' / 'cv_ml') ------------ */
/* Per-observation sums of the CV objectives at bandwidths bw (SM:kernel_density.py:126-160,246-332;
 * the reference's caller: kde.py:145-147):
 *   F[i] = sum_j prod_d kbar_d(X_j, X_i) / bwprod     (convolution kernels; imse's first term)
 *   L[i] = sum_{j != i} prod_d k_d(X_j, X_i) / bwprod (leave-one-out kernels)
 * imse = sum_i F[i] / n^2 - 2 sum_i L[i] / (n (n-1)); loo log-likelihood = -sum_i log L[i] (host sums,
 * in order).  X: device f64[n][D]; vartype: device i32[D] (0 = 'c', 1 = 'u'); bw: device f64[D];
 * lev/lev_off: device, per categorical dim d the ascending unique values of -X[:, d] in
 * lev[lev_off[d] .. lev_off[d+1]) (continuous dims: empty); loo_levels: device i32[n][D], the level
 * count of column d without row i; c4 = 1/sqrt(4 pi), c2 = 1/sqrt(2 pi), bwprod = prod of the
 * continuous bandwidths in dim order (host).  F or L may be NULL (not computed). */
int hbx_kde_cv_terms(const double* X, int64_t n, int32_t D, const int32_t* vartype, const double* bw,
                     const double* lev, const int32_t* lev_off, const int32_t* loo_levels, double c4, double c2,
                     double bwprod, double* F, double* L, void* stream);

/* ---- multi-GPU winner exchange (candidate sharding; bohb.py:133-152 sharded) ----- */
/* Each rank runs hbx_kde_acquire on its contiguous shard with index_base = its first global index; the
 * ranks' result records then meet in ONE RCCL all-gather over xGMI and are reduced on the device by
 * (score, global index): the smallest score, ties to the smallest index -- the reference's strict '<'
 * in index order.  Winners within each other's error bounds set HBX_ACQ_NEAR_TIE (record.near = ranks
 * involved) for a host re-resolution.  ("argmax" of l/g = argmin of the BOHB score g/l.)
 *   local: this rank's device result record (hbx_kde_result_ptr); gather: device scratch of
 *   hbx_argmax_gather_bytes(nranks) holding every rank's record afterwards; out: device record of the
 *   global winner; rccl_comm: an ncclComm_t (hbx_rccl_comm_init, or the caller's own). */
int64_t hbx_rccl_unique_id_bytes(void);
int hbx_rccl_get_unique_id(void* id_out);
int hbx_rccl_comm_init(void** comm, int32_t nranks, const void* id, int32_t rank, int32_t device);
/* the communicator's rank count as RCCL reports it (ncclCommCount) */
int hbx_rccl_comm_count(void* comm, int32_t* count);
int hbx_rccl_comm_destroy(void* comm);
int64_t hbx_argmax_gather_bytes(int32_t nranks);
int hbx_argmax_allreduce(const void* local, void* gather, void* out, int32_t nranks, void* rccl_comm, void* stream);
/* The same reduction over records gathered by another transport (device AcqResult[nranks] -> out). */
int hbx_argmax_records(const void* all, int32_t nranks, void* out, void* stream);

/* ---- successive-halving promotion -------------------------------------------------------- */
/* advance[i] = rank_i < k[b] among the finite losses of bracket b (non-finite = CRASHED, never
 * advance; ties ranked by position).  loss: device f64[N]; seg_off: device i64[B+1]; k: device f64[B];
 * order: device i64[N] (sorted positions per bracket, output) or NULL when only the mask is wanted --
 * brackets of <= 1024 configurations then take an O(n) selection of the k-th loss and need no
 * scratch (scratch may be NULL); advance: device u8[N]; n_advance: device i64[B], nullable.
 * scratch: hbx_sort_scratch_bytes(N) bytes when order is requested or a bracket exceeds 1024.
 * N = 0 (every bracket empty): loss, order and advance may be NULL; n_advance is zeroed. */
int hbx_sh_promote(const double* loss, const int64_t* seg_off, int64_t B, int64_t max_seg, int64_t N,
                   const double* k, int64_t* order, uint8_t* advance, int64_t* n_advance, void* scratch,
                   int64_t scratch_bytes, void* stream);

/* hbx_sh_promote with the tie order chosen (hbx_sh_promote itself = HBX_ORDER_STABLE).  HBX_ORDER_NUMPY:
 * the finite losses of a bracket are ranked in numpy's argsort order (HB_iteration.py:179-180 sees only
 * the REVIEW configurations); brackets whose tied losses straddle the k-th place (or, with `order`
 * requested, hold any tie) are re-ranked on the device.  scratch: hbx_sh_promote_scratch_bytes(...)
 * bytes (never NULL in HBX_ORDER_NUMPY). */
int64_t hbx_sh_promote_scratch_bytes(int64_t B, int64_t max_seg, int64_t N, int32_t order_requested,
                                     int32_t order_mode);
int hbx_sh_promote_ex(const double* loss, const int64_t* seg_off, int64_t B, int64_t max_seg, int64_t N,
                      const double* k, int64_t* order, uint8_t* advance, int64_t* n_advance, void* scratch,
                      int64_t scratch_bytes, int32_t order_mode, void* events, void* stream);
/*   events: NULL, or hipEvent_t[2] stamped at the start and end of the selection kernel (mask-only path). */

/* One bracket of n <= 1024 configurations (what SuccessiveHalving.process_results ranks per call,
 * HB_iteration.py:179-182): a one-wave selection launch, then (HBX_ORDER_NUMPY) a re-rank launch that works
 * only when tied losses straddle the k-th place.  loss f64[n] and advance u8[n] may be device pointers or
 * mapped host memory from hbx_host_alloc (no copies); k by value; scratch: device int32[4 n]
 * (HBX_ORDER_NUMPY), or NULL (HBX_ORDER_STABLE).  done (nullable, mapped host memory): set to `seq` once
 * every mask byte is visible to the host, so a caller may poll it instead of synchronising the stream. */
int hbx_sh_promote_one(const double* loss, int64_t n, double k, uint8_t* advance, void* scratch, int32_t order_mode,
                       int32_t* done, int32_t seq, void* stream);
/* The same ranking step as ONE host call (what the drop-in's advance_mask makes): losses (host f64[n]) are
 * copied into `pin` (hbx_host_alloc, >= n doubles), the selection runs with advance = `pout`
 * (hbx_host_alloc, >= n bytes), the host spins on `done` (mapped, after pout) until the kernel stores
 * `seq` (> 0; bounded: then the stream is synchronised) -- or -seq: a straddling tie, the re-rank is
 * launched and waited for the same way -- and the mask is copied into `mask` (host u8[n]).
 * losses == pin (filled by the caller) and mask == pout (read by the caller) skip those copies.
 * Replaces np.argsort(np.argsort(losses)) < k of HB_iteration.py:179-182 for one bracket. */
int hbx_sh_advance_mapped(const double* losses, int64_t n, double k, uint8_t* mask, double* pin, uint8_t* pout,
                          int32_t* done, int32_t seq, void* scratch, int32_t order_mode, void* stream);
/* hbx_sh_advance_mapped with its buffers in a state block (4 arguments: what a per-call FFI hop costs, the
 * drop-in's advance_mask pays on every bracket): state = int64[7] {pin, pout, done, scratch, order_mode,
 * seq, device}.  The caller has written the losses into pin; the mask is left in pout; seq is advanced by
 * the call (1 ... 2^31 - 2, wrapping).  The launch runs on `device` (the scratch's; the stream must be one
 * of its streams) whichever device is current on the calling thread, which is left as it was. */
int hbx_sh_advance_state(int64_t* state, int64_t n, double k, void* stream);
/* Pinned, device-mapped, coherent host memory (hipHostMalloc) and its release. */
int hbx_host_alloc(int64_t bytes, void** out);
int hbx_host_free(void* p);

/* Grouped successive halving: the next stage of B brackets from their promotion masks (HB_iteration.py:184-188 the
 * survivors in config-id order, :135-138 new configurations where crashed runs left slots empty).  Bracket b owns the
 * positions seg_off[b] .. seg_off[b+1] of rows (f64[N][D]) and of advance (u8[N], the mask hbx_sh_promote_ex writes;
 * any non-zero byte is set); a_b is its number of set bytes.  rows_out[b][j][0..D) and src_out[b][j], slot j of K:
 *   j < min(a_b, K)                      the row of the j-th set position in ascending position, copied bit for bit;
 *                                        src = that position relative to seg_off[b]
 *   the next f_b = min(F, K - min(a_b, K))  fresh[b][i][0..D), i = 0 .. f_b - 1, copied bit for bit; src = -1 - i
 *                                        (fresh: f64[B][F][D] or NULL, then f_b = 0)
 *   the rest                             every element the quiet NaN 0x7FF8000000000000; src = INT32_MIN
 * counts_out (i64[B][2], nullable): {a_b, f_b}, a_b the true count also where it exceeds K.  Values are never
 * interpreted (NaN payloads, -0.0, infinities and subnormals move as bits).  seg_off: device i64[B+1], non-decreasing;
 * it is read on the device only.  8-byte alignment of the f64 / i64 pointers suffices (4 for src_out): 16-byte accesses
 * are used only where the kernel finds D even and rows, fresh and rows_out 16-byte aligned.  Nothing outside
 * rows_out[B][K][D], src_out[B][K] and counts_out[B][2] is written, and rows_out is also the call's scratch before
 * its rows are stored.  One launch (brackets up to 8192 positions, or B > 1024: one workgroup per bracket) plus, for
 * B <= 1024, three launches that cut longer brackets into slices (count, rank, gather), all on `stream`; no host
 * synchronisation, no workspace.  B == 0 or K == 0: nothing to do, success.  A bracket longer than 2^31 - 1 positions
 * is undefined.  Null required pointers, D outside [1, hbx_max_dims()], negative B, K or F (or one beyond int32),
 * F > 0 with fresh == NULL, misaligned pointers: HBX_ERR_ARG (hbx_last_error), before anything is launched. */
int hbx_sh_advance_groups(const double* rows, int32_t D, const int64_t* seg_off, int64_t B, const uint8_t* advance,
                          const double* fresh, int64_t F, int64_t K, double* rows_out, int32_t* src_out,
                          int64_t* counts_out, void* stream);

/* ---- numpy's argsort on the host (hbx_npsort_host.cpp) ------------------------------------------------
 * hbx_np_argsort_host: np.argsort(x) of numpy 1.26.4 on an AVX-512 host (x86-simd-sort avx512_argsort<double>,
 *   std::sort with NaN last when a NaN is present), ties in its order; host x[n] -> host order[n].
 * hbx_sh_advance_host: one bracket's HB_iteration.py:180-182 on the host: advance[i] = argsort(argsort(loss))[i]
 *   < k, i.e. the first k positions of that argsort; host loss[n], advance u8[n], scratch i64[n].
 *   Replaces np.argsort(np.argsort(losses)) < num_configs[SH_iter] of SuccessiveHalving.process_results for
 *   one bracket whose tied losses straddle the k-th place (hbx_sh_promote_ex ranks batched brackets). */
int hbx_np_argsort_host(const double* x, int64_t n, int64_t* order);
int hbx_sh_advance_host(const double* loss, int64_t n, int64_t k, uint8_t* advance, int64_t* scratch);

/* ---- BOHB's candidate draws on the host (bohb.py:133-147), the reference's RNG stream -------------
 * Host code (hbx_draw.cpp), no device work.  `state` is the MT19937 state a legacy numpy RandomState
 * holds (uint32 key[624] followed by int pos: hbx_mt_state_bytes() bytes, e.g. the global generator's
 * bit_generator.ctypes.state_address, held under that generator's lock); the draws continue its stream
 * exactly as the reference's calls would.
 * hbx_mt_draw: n draws of random_sample() (kind 0) or randint(0, high) (kind 1) into out (self-checks).
 * hbx_bohb_draw: one get_config call's draws -- per candidate randint(0, n) for the datum (bohb.py:135),
 *   then per dim of data[idx] (host f64[n][D]): levels[d] == 0 (continuous): scipy truncnorm.rvs's domain
 *   check (a = -m/bw < b = (1-m)/bw, scale = bw_factor bw >= 0; on failure *stop = element, return 1, the
 *   state left as the reference's raise leaves it), loc returned when scale == 0, else ONE uniform into
 *   uni[e] with need_ppf[e] = 1 and vals[e] = m (the caller computes truncnorm._ppf(uni, a, b) * scale + m,
 *   the rest of rvs); levels[d] > 0: rand() < 1 - bw keeps m, else randint(levels[d]) (bohb.py:144-147).
 *   vals/uni: host f64[num_samples][D]; need_ppf: host u8[num_samples][D]; datum: host i64[num_samples]
 *   (nullable).  compact (nullable, host i64[2][num_samples D]): instead of need_ppf, the inversion's inputs
 *   packed in draw order -- uni[j] the j-th uniform, compact[j] its element index i D + d, compact[num_samples
 *   D + j] its term index datum D + d -- and *n_compact = their count (need_ppf then nullable).
 *   Replaces the scalar draw loop of bohb.py:133-147 (the scoring moved to hbx_kde_acquire). */
int64_t hbx_mt_state_bytes(void);
int hbx_mt_draw(void* state, int32_t kind, int64_t n, int64_t high, double* out);
int hbx_bohb_draw(void* state, const double* data, int64_t n, int32_t D, const double* bw, const int64_t* levels,
                  double bw_factor, int64_t num_samples, double* vals, double* uni, uint8_t* need_ppf,
                  int64_t* datum, int64_t* stop, int64_t* compact, int64_t* n_compact);

#ifdef __cplusplus
}
#endif

#endif /* HBX_H_ */
