// hbx_refit.hip -- the one-call refit on MI355X (gfx950) (BOHB.new_result, bohb.py:211-251): append the new
// rows, sort the losses, fit both KDEs' bandwidths (hbx_fit.hip) and prepare both for scoring (hbx_prep.hip),
// enqueued without host synchronisation.  hbx_kde_refit_sync also brings the output block to the host through a
// device-mapped buffer (hbx_host.h).
#include <string.h>

#include "hbx_host.h"
#include "hbx_prep.h"

// Split metadata hbx_seg_argsort / hbx_kde_fit read from device memory, written by a kernel from its
// arguments (no host copy).
static size_t refit_meta_bytes() { return (sizeof(RefitMeta) + 255) & ~(size_t)255; }

// Append the n_new staged rows ([n_new][D] then n_new losses) at rows n - n_new .. n - 1 of X / loss,
// and write the split metadata (block 0).
__global__ __launch_bounds__(256) void kde_refit_meta_kernel(double* __restrict__ X, double* __restrict__ loss,
                                                             const double* __restrict__ staged, int64_t n_new,
                                                             RefitMetaArgs a, RefitMeta* __restrict__ m) {
  const int64_t per = n_new * (int64_t)a.D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < per + n_new; e += (int64_t)gridDim.x * 256) {
    if (e < per) X[(a.n - n_new) * (int64_t)a.D + e] = staged[e];
    else loss[a.n - n_new + (e - per)] = staged[e];
  }
  if (blockIdx.x == 0) {
    for (int d = threadIdx.x; d < a.D; d += 256) m->vt[d] = (a.vt[d >> 5] >> (d & 31)) & 1u;
    if (threadIdx.x == 0) {
      m->seg[0] = 0;
      m->seg[1] = a.n;
      m->n_good = a.n_good;
      m->n_bad = a.n_bad;
      m->fac_good = a.fac_good;
      m->fac_bad = a.fac_bad;
    }
  }
}

// output block of hbx_kde_refit: order i64[n] | bw_good f64[D] | bw_bad f64[D] | nlev_good i32[D] |
// nlev_bad i32[D] | info_good i32[8] | info_bad i32[8]
struct RefitOut {
  size_t order, bw_good, bw_bad, nlev_good, nlev_bad, info_good, info_bad, total;
};
static RefitOut refit_out_layout(int64_t n, int32_t D) {
  RefitOut o;
  o.order = 0;
  o.bw_good = 8 * (size_t)n;
  o.bw_bad = o.bw_good + 8 * (size_t)D;
  o.nlev_good = o.bw_bad + 8 * (size_t)D;
  o.nlev_bad = o.nlev_good + 4 * (size_t)D;
  o.info_good = o.nlev_bad + 4 * (size_t)D;
  o.info_bad = o.info_good + 32;
  o.total = o.info_bad + 32;
  return o;
}

extern "C" {

int64_t hbx_kde_refit_out_bytes(int64_t n, int32_t D) { return (int64_t)refit_out_layout(n, D).total; }
int64_t hbx_kde_refit_scratch_bytes(int64_t n, int32_t D) {
  // metadata | sort scratch | host rows staged to the device (hbx_kde_refit_sync, beyond the inline copy)
  return (int64_t)refit_meta_bytes() + ((hbx_sort_scratch_bytes(n) + 15) & ~(int64_t)15) + 8 * n * ((int64_t)D + 1);
}

}  // extern "C"

// hbx_kde_refit / hbx_kde_refit_sync (staged_host: the appended rows are in host memory)
static int refit_impl(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype, const double* staged,
                      bool staged_host, int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good, double fac_bad,
                      void* params_good, float* table_good, int64_t table_good_floats, void* params_bad,
                      float* table_bad, int64_t table_bad_floats, void* out, void* scratch, int64_t scratch_bytes,
                      void* stream, const hbx_rules* rules, const PrepPub* pub = nullptr) {
  if (const int rrc = hbx_rules_check("hbx_kde_refit", rules)) return rrc;
  if (!X || !loss || !vartype || !params_good || !table_good || !params_bad || !table_bad || !out || !scratch ||
      (n_new > 0 && !staged))
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_refit: null pointer");
  if (D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_UNSUPPORTED, "D=%d outside [1, %d]", D, HBX_MAX_D);
  if (n < 1 || n > INT32_MAX || n_new < 0 || n_new > n)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_refit: n=%lld, n_new=%lld", (long long)n, (long long)n_new);
  if (n_good < 1 || n_good > n || n_bad < 1 || n_bad > n)
    return hbx_fail(HBX_ERR_ARG, "hbx_kde_refit: split %lld / %lld of %lld rows", (long long)n_good,
                    (long long)n_bad, (long long)n);
  if (scratch_bytes < hbx_kde_refit_scratch_bytes(n, D)) return hbx_fail(HBX_ERR_ARG, "refit scratch too small");
  hipStream_t s = (hipStream_t)stream;
  const RefitOut o = refit_out_layout(n, D);
  char* ob = (char*)out;
  int64_t* order = (int64_t*)(ob + o.order);
  double* bw_g = (double*)(ob + o.bw_good);
  double* bw_b = (double*)(ob + o.bw_bad);
  int32_t* nl_g = (int32_t*)(ob + o.nlev_good);
  int32_t* nl_b = (int32_t*)(ob + o.nlev_bad);
  PrepSet ps;
  memset(&ps, 0, sizeof(ps));
  ps.nk = 2;
  int rc = prep_args(&ps.k[0], X, D, order, (int32_t)n_good, vartype, bw_g, nl_g, params_good,
                     (int32_t*)(ob + o.info_good), table_good_floats);
  if (rc) return rc;
  rc = prep_args(&ps.k[1], X, D, order + (n - n_bad), (int32_t)n_bad, vartype, bw_b, nl_b, params_bad,
                 (int32_t*)(ob + o.info_bad), table_bad_floats);
  if (rc) return rc;
  if (pub) {  // the finishing blocks publish the output block (word offsets of the layout above)
    ps.pub = *pub;
    ps.pub.src = (const uint32_t*)out;
    ps.pub.n = (int32_t)n;
    ps.pub.bw_off[0] = (int32_t)(o.bw_good / 4);
    ps.pub.bw_off[1] = (int32_t)(o.bw_bad / 4);
    ps.pub.nl_off[0] = (int32_t)(o.nlev_good / 4);
    ps.pub.nl_off[1] = (int32_t)(o.nlev_bad / 4);
    ps.pub.info_off[0] = (int32_t)(o.info_good / 4);
    ps.pub.info_off[1] = (int32_t)(o.info_bad / 4);
    ps.pub.D = D;
  }
  RefitMetaArgs ma;
  memset(&ma, 0, sizeof(ma));
  ma.n = n;
  ma.n_good = n_good;
  ma.n_bad = n_bad;
  ma.fac_good = fac_good;
  ma.fac_bad = fac_bad;
  ma.D = D;
  memcpy(ma.vt, ps.k[0].vt, sizeof(ma.vt));
  RefitMeta* m = (RefitMeta*)scratch;
  char* sort_scratch = (char*)scratch + refit_meta_bytes();
  double* stage_dev = (double*)(sort_scratch + ((hbx_sort_scratch_bytes(n) + 15) & ~(int64_t)15));
  const int64_t nst = n_new * ((int64_t)D + 1);  // staged doubles: the rows, then their losses
  // host rows: carried in the sort launch's arguments when they fit (no copy), else copied through the scratch
  const bool inl = staged_host && n <= REFIT_SORT_SMALL && nst <= REFIT_INLINE;
  if (staged_host && !inl && nst > 0) {
    HBX_HIP(hipMemcpyAsync(stage_dev, staged, 8 * (size_t)nst, hipMemcpyHostToDevice, s));
    staged = stage_dev;
  }
  // numpy's argsort order (bohb.py:229): tied losses -- crashed +inf runs, quantised losses -- give the
  // reference's rows in the reference's order
  if (n <= REFIT_SORT_SMALL) {  // one launch: rows appended, metadata, sort, numpy's tie order
    rc = refit_sort_small(X, loss, inl ? nullptr : staged, inl ? staged : nullptr, n_new, ma, m, order,
                          (int32_t*)sort_scratch, s);
    if (rc) return rc;
  } else {
    const int64_t per = n_new * (int64_t)(D + 1);
    const unsigned gmeta = (unsigned)(per > 0 ? ((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024) : 1);
    hipLaunchKernelGGL(kde_refit_meta_kernel, dim3(gmeta), dim3(256), 0, s, X, loss, staged, n_new, ma, m);
    HBX_LAUNCH_CHECK();
    rc = hbx_seg_argsort_ex(loss, m->seg, 1, n, n, order, sort_scratch, hbx_sort_scratch_bytes(n), HBX_ORDER_NUMPY,
                            stream);
    if (rc) return rc;
  }
  // both sets within one LDS tile: the fit also writes the preparation's column statistics (one launch less)
  const bool fused = D > 1 && n_good <= FIT_TILE_ROWS && n_bad <= FIT_TILE_ROWS;
  // (the bandwidths are clipped where the fit stores them: the preparation below reads the clipped ones)
  if (fused)
    rc = refit_fit_colstats(X, D, m->seg, order, &m->n_good, &m->n_bad, &m->fac_good, &m->fac_bad, m->vt, bw_g, bw_b,
                            nl_g, nl_b, col_stats((KdeParams*)params_good), col_stats((KdeParams*)params_bad),
                            rules ? rules->min_bandwidth : 0.0, s);
  else
    rc = hbx_kde_fit_r(X, D, m->seg, 1, order, &m->n_good, &m->n_bad, &m->fac_good, &m->fac_bad, m->vt, bw_g, bw_b,
                       nl_g, nl_b, stream, rules);
  if (rc) return rc;
  return prep_launch(ps, table_good, table_bad, s, fused);
}

extern "C" {

// The whole refit of one budget in one call, enqueued without host synchronisation: append the staged
// rows, stable argsort of the losses, normal-reference bandwidths and level counts of the good (head
// n_good) and bad (tail n_bad) rows, and both KDEs prepared for scoring.  The caller reads `out` back
// once (its info records say which scoring kernel each KDE runs).
int hbx_kde_refit(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype, const double* staged,
                  int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good, double fac_bad, void* params_good,
                  float* table_good, int64_t table_good_floats, void* params_bad, float* table_bad,
                  int64_t table_bad_floats, void* out, void* scratch, int64_t scratch_bytes, void* stream) {
  return hbx_kde_refit_r(X, loss, n, D, vartype, staged, n_new, n_good, n_bad, fac_good, fac_bad, params_good,
                         table_good, table_good_floats, params_bad, table_bad, table_bad_floats, out, scratch,
                         scratch_bytes, stream, nullptr);
}

// hbx_kde_refit with both KDEs' bandwidths clipped from below at rules->min_bandwidth (NULL: no clip)
int hbx_kde_refit_r(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype, const double* staged,
                    int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good, double fac_bad, void* params_good,
                    float* table_good, int64_t table_good_floats, void* params_bad, float* table_bad,
                    int64_t table_bad_floats, void* out, void* scratch, int64_t scratch_bytes, void* stream,
                    const hbx_rules* rules) {
  return refit_impl(X, loss, n, D, vartype, staged, false, n_new, n_good, n_bad, fac_good, fac_bad, params_good,
                    table_good, table_good_floats, params_bad, table_bad, table_bad_floats, out, scratch, scratch_bytes,
                    stream, rules);
}

// hbx_kde_refit with the appended rows in HOST memory (rows then losses, n_new (D + 1) doubles: up to 256
// doubles ride in the first launch's kernel arguments, no copy; more go through the scratch), then the output
// block in host memory (out_host, hbx_kde_refit_out_bytes) when the
// call returns: the preparation's launches publish it to a device-mapped host buffer, every 32-bit word as a
// flagged word carrying the call's sequence number (the parameter launch the rows, bandwidths and level counts,
// the finishing blocks the info records; PrepPub), and the call spins until every word carries it -- no copy
// launch, no stream synchronisation, and no reliance on the order in which the launches' stores reach the host
// (bounded spin: then the stream is synchronised and the words checked once more).  The prepared parameter
// blocks and tables are complete for work on the refit's stream; another stream orders itself after the refit
// with hbx_stream_order (KDEPair does it when the calling stream is not the refit's)
int hbx_kde_refit_sync(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype,
                       const double* staged_host, int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good,
                       double fac_bad, void* params_good, float* table_good, int64_t table_good_floats,
                       void* params_bad, float* table_bad, int64_t table_bad_floats, void* out, void* scratch,
                       int64_t scratch_bytes, void* stream, void* out_host) {
  return hbx_kde_refit_sync_r(X, loss, n, D, vartype, staged_host, n_new, n_good, n_bad, fac_good, fac_bad, params_good,
                              table_good, table_good_floats, params_bad, table_bad, table_bad_floats, out, scratch,
                              scratch_bytes, stream, out_host, nullptr);
}

// hbx_kde_refit_sync with both KDEs' bandwidths clipped from below at rules->min_bandwidth (NULL: no clip)
int hbx_kde_refit_sync_r(double* X, double* loss, int64_t n, int32_t D, const int32_t* vartype,
                         const double* staged_host, int64_t n_new, int64_t n_good, int64_t n_bad, double fac_good,
                         double fac_bad, void* params_good, float* table_good, int64_t table_good_floats,
                         void* params_bad, float* table_bad, int64_t table_bad_floats, void* out, void* scratch,
                         int64_t scratch_bytes, void* stream, void* out_host, const hbx_rules* rules) {
  if (const int rrc = hbx_rules_check("hbx_kde_refit_sync", rules)) return rrc;  // (before the mapped buffer is taken)
  if (!out_host) return hbx_fail(HBX_ERR_ARG, "hbx_kde_refit_sync: null host output");
  if (n < 1 || n > INT32_MAX || D < 1 || D > HBX_MAX_D) return hbx_fail(HBX_ERR_ARG, "hbx_kde_refit_sync: n, D");
  const int64_t words = n + 6 * (int64_t)D;  // flagged words before the info records
  MappedBuf* mb = nullptr;
  int rc = hbx_mapped_refit(8 * words, &mb);
  if (rc) return rc;
  uint64_t* w = (uint64_t*)mb->p;
  uint64_t* ll = (uint64_t*)(mb->p + mb->cap);
  const int32_t seq = mb->seq;
  PrepPub pub;
  memset(&pub, 0, sizeof(pub));
  pub.dst = w;
  pub.ll = ll;
  pub.seq = seq;
  mb->pending = true;
  rc = refit_impl(X, loss, n, D, vartype, staged_host, true, n_new, n_good, n_bad, fac_good, fac_bad, params_good,
                  table_good, table_good_floats, params_bad, table_bad, table_bad_floats, out, scratch, scratch_bytes,
                  stream, rules, &pub);
  if (rc) return rc;
  // the info records come last: spin on them, then every other word (each wait bounded: ~0.1 s, then the
  // stream is synchronised and the words looked at once more)
  const hipStream_t s = (hipStream_t)stream;
  const char* who = "hbx_kde_refit_sync";
  const RefitOut o = refit_out_layout(n, D);
  uint32_t* info = (uint32_t*)((char*)out_host + o.info_good);  // info good | info bad
  uint32_t* rest = (uint32_t*)((char*)out_host + o.bw_good);    // bw good | bw bad | nlev good | nlev bad
  rc = wait_tagged(ll, 16, seq, info, s, 5000000, who);
  if (!rc) rc = wait_tagged(w, n, seq, nullptr, s, 5000000, who);
  if (!rc) rc = wait_tagged(w + n, 6 * (int64_t)D, seq, rest, s, 5000000, who);
  if (rc) return rc;
  mb->pending = false;
  int64_t* order = (int64_t*)out_host;
  for (int64_t i = 0; i < n; ++i) order[i] = (int64_t)(uint32_t)w[i];
  const int32_t* nl = (const int32_t*)((const char*)out_host + o.nlev_good);  // good then bad
  for (int32_t d = 0; d < 2 * D; ++d)
    if (nl[d] < 0) return hbx_fail(HBX_ERR_ARG, "categorical codes must be integers in [0, 1024)");
  return HBX_OK;
}

}  // extern "C"
