// hbx_groups.hip -- grouped acquisition: one exact pick per KDE pair for B independent brackets in two
// launches (hbx_kde_acquire_groups; bohb.py:124-169 per bracket, after the batched refit bohb.py:220-246), and one
// per get_config request when a bracket issues S of them (hbx_kde_acquire_groups_batch, below).
//
// Inputs are hbx_kde_fit's, as they lie on the device: group b's rows are X[seg_off[b] + order[seg_off[b] + j]],
// good KDE j < n_good[b], bad KDE j in [n - n_bad[b], n); its bandwidths and level counts are bw_*[b][D],
// nlev_*[b][D]; its candidate pool is cand[b][C][D].  No KdeParams, no prepared table, no prepare step, no host
// synchronisation: every per-group constant is derived inside the kernels.
//
// Launch 1, groups_screen_kernel<DCP, DUP, NW, DT>: grid = B x ceil(C / 64) linear in blockIdx.x, NW waves.
//   Lane = candidate (its scaled coordinates in registers), the block's waves take the KDE's 64-observation
//   chunks in turn (wave w: chunks w, w + NW, ...), each staged into the wave's LDS rows as fp32 and read back as
//   broadcasts.  Per pair, in log2 units (fp32, direct differences -- no expansion, so no cancellation):
//     t_ij = lb + sum_c -(a_ic - b_jc)^2 + sum_u m_iju delta_u,      a = fl(s_c (x_c - mu_c)), b = fl(s_c (X_jc - mu_c))
//   s_c = sqrt(log2 e / 2) / h_c, mu_c = mean of the group's first <= 64 good rows (any centre is exact algebra; this
//   one keeps |a|, |b| small), m = [x_u == X_ju], lb = sum_u log2(h_u / (c_u - 1)), delta_u = log2|1 - h_u| - log2(h_u /
//   (c_u - 1)) (-1e30 where 1 - h_u == 0: the term is exactly 0).  A categorical h > 1 makes the match factor negative:
//   the term's sign is the parity of its matches in such dims, and positive and negative terms are summed apart.
//   Running log-sum-exp per lane with an INTEGER running maximum m = max ceil(t): the sums S+-, in units of 2^m,
//   are rescaled by ldexp (exact), each term adds exp2(t - m).  No static offset, no underflow, no rescue pass.
//   The waves' (m, S+, S-) meet in LDS and merge by ldexp.  Output per candidate: KdeEst {ln S+, ln S-, err} per
//   KDE (the normalisation -ln n - sum_c ln(h_c sqrt(2 pi)) added in fp64) -> score_interval() (hbx_acq_impl.h)
//   unchanged -> GScreen {slo, shi, rel, flags} in the workspace.
//   The slot bucket is picked by the host from D alone (vartype is device memory): D <= 8, 16, 32 -> every dim
//   may be of either kind (DCP = DUP = the bucket); D <= 96 -> up to 64 continuous and 32 categorical.  Inside a
//   bucket, dc <= 32 with du <= 8 (config #5: 24c + 8u) runs a loop without branches, its piece counts compile-time;
//   everything else a loop with a uniform branch per 4-slot piece (grp_pair_t's two forms, hbx_groups_impl.h).
//   Staging (grp_stage): lane = (row in pass, dim), so a row's D doubles are read by consecutive lanes, 16 passes of
//   loads in flight; the chunk's row positions come in one coalesced load and reach the lanes by a lane exchange.
//   The classification, the slots, the row layout, the per-group constants, the staging, the pair chain, the bound
//   and the GScreen record are hbx_groups_impl.h's, shared with the tile screen and the grouped ln-pdf; the derivation
//   of the error bound (E_t, err = 1.05 E_t + (2 n + 40) u) stands there, with the code it describes.
//
// Launch 2, groups_select_kernel: one block per group (per request, below).  U = min shi over the certified candidates; the shortlist
//   is {slo <= U} plus the uncertified ones, and of the candidates whose score is certainly exactly 1 (both pdfs
//   certainly below the score floor, GrpArgs.F) only the first index.  Every shortlisted candidate gets both exact fp64 pdfs
//   in the reference's arithmetic (hbx_exact_impl.h: the single path's functions, fed a per-group parameter view),
//   then bohb_score, the strict argmin by (score, index), near_best and the record.  A group is exact-only (every
//   candidate re-scored, HBX_ACQ_OVERFLOW) when a continuous bandwidth is not a positive finite number, a
//   categorical dim has a single level (c == 1; h == 0, or h > 0 and finite), the dims exceed the bucket, or a pdf bound
//   leaves fp64's exp range.  Correctness never rests on the screen: it only decides what is re-scored.
//   The exact scores are kept in the candidates' GScreen slots for the near-tie count (no second buffer).
//
// S requests per group (hbx_kde_acquire_groups_batch; bohb.py:124-169 once per get_config call of a stage,
// HB_iteration.py:136-138): cand is [B][S][C][D], request q = b S + s has its own pool, its own record q and its own
// select block (grid B S: screen slots from q C, candidates from q C D; U, the first certain 1, the shortlist, the
// argmin and the near count never leave the request).  The screen is per candidate, so it sees group b's S C
// candidates as one flattened pool P of ceil(S C / 64) tiles (a tile may straddle two requests).  Which screen runs
// is grp_tile_screen()'s rule, in one place: S == 1 is hbx_kde_acquire_groups itself, launch 1 above; from
// GRP_TILES_MIN tiles per group on, the tile screen below; under that, launch 1 over the flattened pool.
//
// The tile screen, groups_tiles_kernel<DCP, DUP, NW, DT>: grid = B x slabs, a block is one group and a slab of NW
//   of its tiles (slabs = ceil(tiles / NW)); wave w owns tile tile0 + w, lane = candidate.  Every wave walks every
//   chunk of a KDE for its own candidates: no partial sums, no merge.  The group's status, slots, centres, scales,
//   lb, deltas and norms are derived once per block and serve the slab's NW tiles.  (Slabs of 2, 4 and 8 tiles per
//   wave -- the rows walked again per tile, the constants shared further -- measured within 0.8 % of one tile per
//   wave either way; the loop over them is not kept.)  The rows of the good, then the bad KDE
//   form one stream of chunks of 32 NW rows;
//   chunk g lives in LDS buffer g & 1, each wave stages 32 of its rows exactly as in launch 1 (gather through
//   `order`, centred, scaled, fp32).  One barrier per chunk: past barrier g, chunk g is complete and chunk g - 1 is
//   read by everyone, so each wave first stages its rows of chunk g + 1 into the other buffer and then runs its
//   candidates against chunk g -- a wave's gather is in flight while the other waves of the SIMD do pairs.  The two
//   buffers together are launch 1's LDS rows.  s_bmax is kept per KDE: every row of a KDE is staged before the last
//   barrier of its walk and the bound is formed after that barrier (the bad KDE's first chunk, staged meanwhile,
//   goes to its own maxima) -- so a candidate's bound does not depend on timing.
//   Error bound: E_t is launch 1's, term for term (same a, b, dd, fma chain, same T with B_c from s_bmax).  The sum:
//   one lane adds the n terms of a KDE in row order into one running (m, S+, S-); rescaling is exact, each term
//   carries 0.372 u + 2 u e, each addition u, so the sum is within (2 + 0.75 n) u + n u <= (2 n + 40) u -- launch 1's
//   allowance with its 32 u for the merge left unused.  err = 1.05 E_t + (2 n + 40) u as above.
//   The screens' sums differ in the last bits (another order of additions), so shortlist / near / rel may differ
//   between them; index, score and the pdfs come from the fp64 re-score and do not.
//
// The k best candidates per group (hbx_kde_acquire_groups_topk): launch 1 as above, then groups_topk_kernel in
// launch 2's place -- the k-th smallest upper bound, the shortlist against it, the same re-score, and the ranking of
// hbx_topk_rank.h (shared with hbx_topk.hip).  Its comment, before the kernel, has the steps and the argument why the
// shortlist holds the whole top-k.
//
// The grouped sampler (hbx_kde_sample_groups) lives in hbx_sample.hip beside the draw functions it shares with
// hbx_kde_sample, so the byte-equality of the draws holds by construction.
//
// Where this departs from the plan it was built to, and why:
//   - a block's waves split the observation chunks between them instead of all reading each chunk: at C = 64 (the
//     reference's num_samples, config #5) a group has one wave of candidates, and sharing chunks would leave three
//     of the four waves without work; larger pools simply take more 64-candidate blocks;
//   - the slot bucket comes from D alone, and the kernel sorts the dims into slots itself: vartype is device memory
//     and reading it on the host would be the synchronisation the call must not make;
//   - C == 0 launches one small kernel: the B empty records have to be written by something (NaN is not a byte fill).
#include "hbx_groups_impl.h"
#include "hbx_topk_rank.h"

// The acquisition's reading of grp_classify's bits (hbx_groups_impl.h), stated here and nowhere else: a group is
// exact-only -- re-scored whole, HBX_ACQ_OVERFLOW -- when either of its KDEs cannot be screened (GRP_EXACT(kd)); a
// negative match factor (h > 1, GRP_NEG(kd)) is screened like any other KDE, as a signed sum.
#define GRP_EXACT_ONLY GRP_EXACT_ANY
#define GRP_NO_SCREEN (GRP_NO_MODEL | GRP_UNSUPPORTED | GRP_EXACT_ONLY)

struct GrpArgs {
  GrpModel M;
  const double* cand;
  int64_t S, C;      // requests per group (1: hbx_kde_acquire_groups), candidates per request
  int64_t P;         // S * C: the group's flattened pool, what the screen sees
  int32_t tiles;     // ceil(P / 64)
  int32_t slabs;     // tile screen: blocks per group, one tile per wave
  GScreen* scr;
  AcqResult* res;
  ScoreFloor F;      // the call's score floor (hbx_rules.pdf_floor), read by the kernels' <.., DEFF = false> instances
  // the request mask (hbx_kde_acquire_groups_batch_m), read by the kernels' <.., MASK = true> instances alone:
  const uint8_t* want;         // u8[B][S], request (b, s) is answered when its byte is not 0; NULL: every request
  unsigned long long* stats;   // the workspace head's four counters (hbx_kde_groups_request_stats)
};

// The request mask in a kernel.  MASK follows DEFF's precedent: the <.., MASK = false> instances are, instruction for
// instruction, the kernels the unmasked entry points have always launched (profiles/request_mask/README.md has the
// register figures of both); the <.., true> instances serve hbx_kde_acquire_groups_batch_m.  The grid is the dense
// one either way -- the host never reads the mask -- and blocks and waves decide for themselves:
//   groups_screen_kernel   a tile of the flattened pool without a wanted candidate returns after its uniform test,
//                          before classification and staging; in a mixed tile the lanes of unwanted requests are !valid
//   groups_tiles_kernel    the block lists its group's wanted tiles (grp_wanted_tiles) and slab j takes the wanted
//                          tiles j NW .. j NW + NW - 1; slabs beyond the list return at once
//   groups_select_kernel   the block of an unwanted request classifies its group, writes the skipped record, returns
// A candidate's arithmetic does not change with the mask (the same rows in the same order into the same sums), and
// the host picks the screen from the dense S and tile count, so a wanted request's record is the dense call's, byte
// for byte.  Counters, one atomic add per block: [0] requests answered, [1] requests skipped (select), [2] candidates
// the screen evaluated, [3] candidates re-scored in fp64 (select).
__device__ __forceinline__ bool grp_wanted(const GrpArgs& A, int64_t b, int64_t i) {  // candidate i of group b's pool
  return !A.want || A.want[b * A.S + (int64_t)((uint32_t)i / (uint32_t)A.C)] != 0;    // (i < P <= INT32_MAX)
}

// The wanted tiles of group b in ascending order, ranks r0 .. r0 + NW - 1, into s_tile[0 .. NW) (-1 past the list):
// one wave, 64 tiles per round -- lane = tile, wanted when a request that owns one of its candidates is, a ballot
// prefix gives its rank.  Stops once the slab is full.
template <int NW>
__device__ __forceinline__ void grp_wanted_tiles(const GrpArgs& A, int64_t b, int r0, int lane, int32_t* s_tile) {
  if (lane < NW) s_tile[lane] = -1;
  int cnt = 0;
  for (int t0 = 0; t0 < A.tiles && cnt < r0 + NW; t0 += 64) {  // (uniform)
    const int t = t0 + lane;
    bool w = false;
    if (t < A.tiles) {
      const int64_t i0 = (int64_t)t * 64, i1 = i0 + 63 < A.P ? i0 + 63 : A.P - 1;
      if (!A.want) {
        w = true;
      } else {
        const int s1 = (int)((uint32_t)i1 / (uint32_t)A.C);
        for (int s = (int)((uint32_t)i0 / (uint32_t)A.C); s <= s1; ++s) w = w || A.want[b * A.S + s] != 0;
      }
    }
    const uint64_t bal = __ballot(w);
    const int r = cnt + __popcll(bal & ((1ull << lane) - 1ull)) - r0;
    if (w && r >= 0 && r < NW) s_tile[r] = t;
    cnt += __popcll(bal);
  }
}

// The call's score floor in a kernel.  DEFF: the reference snapshot's 1e-8 as compile-time constants
// (hbx_score_floor(1e-8)'s values) -- the default path's kernels are then instruction for instruction what they were
// before the floor became a parameter (read from the arguments, the same arithmetic measured 0.5 % slower on the
// grouped benchmark: another register allocation of the screen, profiles/rules/README.md); else the launch argument.
template <bool DEFF>
__device__ __forceinline__ ScoreFloor grp_floor(const GrpArgs& A) {
  if constexpr (DEFF)
    return ScoreFloor{HBX_PDF_FLOOR_DEFAULT, (float)HBX_LN_CLAMP, (float)HBX_LN_CLAMP - 1e-4f, 0.f};
  else
    return A.F;
}

// the dispatch's call: this lane's candidate against jmax staged rows, piece counts (QC, QU), signed or not
#define GRP_PAIRS_CALL(QC, QU, SG) \
  grp_pairs<DCP, DUP, QC, QU, SG>(srows, L.rs, jmax, L.dcq, L.duq, xc, xu, dl, nf, lbs, m, sp, sn)

template <int DCP, int DUP, int NW, int DT, bool DEFF, bool MASK>
__global__ __launch_bounds__(64 * NW) void groups_screen_kernel(GrpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  GRP_SCREEN_CONSTS_LDS(K, DCP, DUP);
  __shared__ uint32_t s_bmax[DCP];
  __shared__ float s_pm[NW][64], s_ps[NW][64], s_pn[NW][64];
  __shared__ int32_t s_i[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GrpModel& mod = A.M;
  const int D = mod.D;
  const int64_t b = (int64_t)blockIdx.x / A.tiles;
  const int tile = (int)((int64_t)blockIdx.x - b * A.tiles);
  const int64_t i = (int64_t)tile * 64 + lane;
  bool valid = i < A.P;  // (the group's flattened pool: S requests of C candidates)
  int nvalid = 0;
  if constexpr (MASK) {  // (every wave sees the same 64 candidates: the test is uniform over the block)
    valid = valid && grp_wanted(A, b, i);
    nvalid = __popcll(__ballot(valid));
    if (nvalid == 0) return;
  }
  GScreen* out = A.scr + b * A.P + i;
  if (wave == 0) {
    int dc, du;
    const int st = grp_classify(mod, b, &dc, &du);
    if (lane == 0) {
      s_i[0] = st;
      s_i[1] = dc;
      s_i[2] = du;
    }
    if (!(st & GRP_NO_SCREEN)) grp_slots(mod, lane, K.cdim, K.udim, &dc, &du);  // (then dc <= DCP, du <= DUP)
  }
  __syncthreads();
  const int st = s_i[0], dc = s_i[1], du = s_i[2];
  if (st & GRP_NO_SCREEN) {  // no screen: the select kernel re-scores (or skips)
    if (wave == 0 && valid) *out = grp_uncertified(D, st);
    return;
  }
  if constexpr (MASK)
    if (tid == 0) atomicAdd(A.stats + 2, (unsigned long long)nvalid);
  const int64_t s0 = mod.seg_off[b], n = mod.seg_off[b + 1] - s0;
  const int64_t ng = mod.n_good[b], nb = mod.n_bad[b];
  const double* Xs = mod.X + s0 * D;
  const int64_t* ord = mod.order + s0;
  const GrpLayout L = grp_layout<DCP, DUP>(D, dc, du);
  for (int e = tid; e < NT * L.rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  grp_consts_fill<NT>(K, mod, b, 0, dc, du, L.dc4, tid);
  __syncthreads();
  grp_screen_sums(K, dc, du, ng, nb, tid);
  __syncthreads();
  const double* x = A.cand + (b * A.P + (valid ? i : (int64_t)tile * 64)) * D;
  bool certified = true;
  KdeEst est_l = kde_est_neutral(), est_g = kde_est_neutral();
#pragma unroll 1
  for (int kd = 0; kd < 2; ++kd) {
    const int64_t nk = kd ? nb : ng;
    const int64_t* rows = ord + (kd ? n - nb : 0);
    const int cat = du == 0 ? 0 : (st & GRP_NEG(kd)) ? 2 : 1;
    float xc[DCP], xu[DUP], dl[DUP], nf[DUP];
    // grp_load_cand's statements, kept apart in this kernel: through the function its instances came out at 173, 204
    // and 256 VGPRs + 4 AGPRs (8, 16, 32 slots) -- a wave per SIMD less in the first and the last -- against 165, 196
    // and 256 + 0 with the loop written here
#pragma unroll
    for (int k = 0; k < DCP; ++k) {
      xc[k] = 0.f;
      if (k < dc) {
        const double xv = x[K.cdim[k]];
        certified = certified && (xv - xv == 0.0);
        xc[k] = (float)(K.scale[kd][k] * (xv - K.mu[k]));
      }
    }
#pragma unroll
    for (int u = 0; u < DUP; ++u) {
      xu[u] = 0.f;
      if (u < du) {
        const double xv = x[K.udim[u]];
        certified = certified && (xv - xv == 0.0);
        xu[u] = cand_code(xv);
      }
      dl[u] = grp_uniform(K.delta[kd][u]);
      nf[u] = K.negf[kd][u];  // (vector registers: 2 DUP uniform values exceed the scalar file)
    }
    const float lbs = grp_uniform(K.lbs[kd]);
    for (int k = tid; k < DCP; k += NT) s_bmax[k] = 0u;
    float m = -INFINITY, sp = 0.f, sn = 0.f;
    float* srows = sobs + (size_t)wave * 64 * L.rs;  // this wave's rows
    for (int64_t c0 = 0; c0 < nk; c0 += (int64_t)NW * 64) {  // uniform trip count: the barriers are block-wide
      __syncthreads();  // (the rows of the previous round are read; s_bmax zeroed)
      const int64_t j0 = c0 + (int64_t)wave * 64;
      const int jmax = (int)(nk - j0 < 64 ? (nk - j0 > 0 ? nk - j0 : 0) : 64);
      if (jmax > 0) grp_stage<16>(Xs, D, rows, j0, jmax, srows, L.rs, L.rpp, dc, K.doff, K.dsc[kd], K.dmu, s_bmax, lane);
      __syncthreads();
      if (jmax > 0) GRP_PAIRS_DISPATCH(DCP, L, cat, GRP_PAIRS_CALL);
    }
    s_pm[wave][lane] = m;
    s_ps[wave][lane] = sp;
    s_pn[wave][lane] = sn;
    __syncthreads();
    // merge the waves' partials (every wave computes the same numbers for its lane)
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, s_pm[w][lane]);
    float Sp = 0.f, Sn = 0.f;
    bool bad = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float mw = s_pm[w][lane];
      bad = bad || mw != mw;  // (fmaxf drops a NaN)
      if (mw > -INFINITY) {
        const int sh = (int)fmaxf(mw - M, -250.f);
        Sp += ldexpf(s_ps[w][lane], sh);
        Sn += ldexpf(s_pn[w][lane], sh);
      }
    }
    const KdeEst e = grp_estimate(K, kd, dc, du, nk, s_bmax, xc, M, Sp, Sn, bad, certified);
    if (kd == 0)
      est_l = e;
    else
      est_g = e;
    __syncthreads();  // (s_pm, s_bmax are rewritten for the bad KDE)
  }
  if (wave == 0 && valid) *out = grp_emit(D, st, certified, est_l, est_g, grp_floor<DEFF>(A));
}

// The tile screen (header: "The tile screen"): the block is a slab of NW tiles of one group, wave w owns tile
// tile0 + w and walks every chunk of both KDEs itself; the chunks are staged once for the block, 32 NW rows at a
// time in two buffers.  Shared with groups_screen_kernel through hbx_groups_impl.h's inlined functions: the
// classification and the slots, the row layout, the per-group constants, the staging of a wave's rows, the candidate's
// registers, the pair loops and their dispatch, the bound and the GScreen.  Kept apart: the two kernels themselves --
// how the chunks are walked, who sums what, and s_bmax (one set here per KDE, so that a candidate's bound does not
// depend on timing).  As one kernel with a compile-time switch the 32-slot instance came out at 256 VGPRs + 4 AGPRs,
// one wave per SIMD instead of two (and the 8-slot instance at 174 instead of 165, two waves instead of three); with
// the steps shared as inlined functions the instances (8 / 16 / 32 / 64+32 slots) stand at 165 / 196 / 256 / 256 VGPRs
// for groups_screen_kernel (before: 165 / 196 / 255 / 256) and 190 / 219 / 235 / 256 for this kernel (180 / 209 / 224 /
// 256), every one at the waves per SIMD it had (3 / 2 / 2 / 1 and 2 / 2 / 2 / 1), no scratch.  The one step that
// groups_screen_kernel does not take from the header is the candidate's load (the comment there has the numbers).
template <int DCP, int DUP, int NW, int DT, bool DEFF, bool MASK>
__global__ __launch_bounds__(64 * NW, DCP <= 32 ? 2 : 1) void groups_tiles_kernel(GrpArgs A) {
  constexpr int NT = 64 * NW;
  __shared__ __align__(16) float sobs[NW * 64 * (DT + 4)];
  GRP_SCREEN_CONSTS_LDS(K, DCP, DUP);
  __shared__ uint32_t s_bmax[2][DCP];
  __shared__ int32_t s_i[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GrpModel& mod = A.M;
  const int D = mod.D;
  const int64_t b = (int64_t)blockIdx.x / A.slabs;
  const int tile0 = (int)((int64_t)blockIdx.x - b * A.slabs) * NW;  // the slab's first tile
  // MASK: wave w's tile is the (tile0 + w)-th WANTED tile of the group (-1: none); a slab past the list returns
  int32_t* s_tile = nullptr;
  if constexpr (MASK) {
    __shared__ int32_t s_wtile[NW];
    s_tile = s_wtile;
    if (wave == 0) grp_wanted_tiles<NW>(A, b, tile0, lane, s_tile);
    __syncthreads();
    if (s_tile[0] < 0) return;  // (uniform)
  }
  if (wave == 0) {
    int dc, du;
    const int st = grp_classify(mod, b, &dc, &du);
    if (lane == 0) {
      s_i[0] = st;
      s_i[1] = dc;
      s_i[2] = du;
    }
    if (!(st & GRP_NO_SCREEN)) grp_slots(mod, lane, K.cdim, K.udim, &dc, &du);  // (then dc <= DCP, du <= DUP)
  }
  __syncthreads();
  const int st = s_i[0], dc = s_i[1], du = s_i[2];
  if (st & GRP_NO_SCREEN) {  // no screen: the select kernel re-scores (or skips)
    if constexpr (MASK) {
      const int64_t iw = (int64_t)s_tile[wave] * 64 + lane;
      if (s_tile[wave] >= 0 && iw < A.P && grp_wanted(A, b, iw)) A.scr[b * A.P + iw] = grp_uncertified(D, st);
    } else {
      const int64_t iw = (int64_t)(tile0 + wave) * 64 + lane;
      if (iw < A.P) A.scr[b * A.P + iw] = grp_uncertified(D, st);
    }
    return;
  }
  const int64_t s0 = mod.seg_off[b], n = mod.seg_off[b + 1] - s0;
  const int64_t ng = mod.n_good[b], nb = mod.n_bad[b];
  const double* Xs = mod.X + s0 * D;
  const int64_t* ord = mod.order + s0;
  const GrpLayout L = grp_layout<DCP, DUP>(D, dc, du);
  for (int e = tid; e < NT * L.rs; e += NT) sobs[e] = 0.f;  // (the padding slots stay 0)
  for (int k = tid; k < 2 * DCP; k += NT) s_bmax[k / DCP][k % DCP] = 0u;
  grp_consts_fill<NT>(K, mod, b, 0, dc, du, L.dc4, tid);
  __syncthreads();
  grp_screen_sums(K, dc, du, ng, nb, tid);
  __syncthreads();
  // The rows of the good, then the bad KDE as one stream of chunks of CH = 32 NW rows: chunk g lies in buffer
  // g & 1, every wave stages 32 of its rows.  One barrier per chunk: past it chunk g is staged and chunk g - 1 is
  // read by every wave, so the waves stage chunk g + 1 into the other buffer and then read chunk g -- a wave's
  // gather of the next chunk overlaps the other waves' pairs of this one.  The candidate's registers are live while
  // the next chunk is staged, so the 32-slot instance keeps 8 loads in flight, not 16.
  constexpr int CW = 32, CH = CW * NW, SL = DCP >= 32 ? 8 : 16;
  auto stage_chunk = [&](int kd, int64_t c, int buf) {
    const int64_t nk = kd ? nb : ng, j0 = c * CH + (int64_t)wave * CW;
    const int jmax = (int)(nk - j0 < CW ? (nk - j0 > 0 ? nk - j0 : 0) : CW);
    if (jmax > 0)
      grp_stage<SL>(Xs, D, ord + (kd ? n - nb : 0), j0, jmax, sobs + ((size_t)buf * CH + (size_t)wave * CW) * L.rs, L.rs,
                    L.rpp, dc, K.doff, K.dsc[kd], K.dmu, s_bmax[kd], lane);
  };
  __syncthreads();  // (s_bmax and the padding slots are zeroed)
  stage_chunk(0, 0, 0);
  int g = 0;
  bool certified = true;
  KdeEst est_l = kde_est_neutral();
  int tw = tile0 + wave;  // this wave's tile
  if constexpr (MASK) tw = s_tile[wave];
  const int64_t iw = (int64_t)tw * 64 + lane;
  bool vw = iw < A.P;
  bool live = tw < A.tiles;  // (wave-uniform; a wave without a tile still stages its rows)
  if constexpr (MASK) {
    live = tw >= 0;
    vw = live && vw && grp_wanted(A, b, iw);
    if (wave == 0) {  // the slab's evaluated candidates, counted by one wave: one atomic add per block
      int nev = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const int64_t ie = (int64_t)s_tile[w] * 64 + lane;
        nev += __popcll(__ballot(s_tile[w] >= 0 && ie < A.P && grp_wanted(A, b, ie)));
      }
      if (lane == 0) atomicAdd(A.stats + 2, (unsigned long long)nev);
    }
  }
  const double* x = A.cand + (b * A.P + (vw ? iw : live ? (int64_t)tw * 64 : 0)) * D;
#pragma unroll 1
  for (int kd = 0; kd < 2; ++kd) {
    const int64_t nk = kd ? nb : ng;
    const int cat = du == 0 ? 0 : (st & GRP_NEG(kd)) ? 2 : 1;
    float xc[DCP], xu[DUP], dl[DUP], nf[DUP];
    grp_load_cand<DCP, DUP>(x, dc, du, K.cdim, K.udim, K.scale[kd], K.mu, K.delta[kd], xc, xu, dl, certified);
#pragma unroll
    for (int u = 0; u < DUP; ++u) nf[u] = K.negf[kd][u];  // (vector registers: 2 DUP uniform values exceed the scalar file)
    const float lbs = grp_uniform(K.lbs[kd]);
    float m = -INFINITY, sp = 0.f, sn = 0.f;
    const int64_t nch = (nk + CH - 1) / CH;
    for (int64_t c = 0; c < nch; ++c, ++g) {  // uniform trip counts: the barriers are block-wide
      __syncthreads();
      if (c + 1 < nch)
        stage_chunk(kd, c + 1, (g + 1) & 1);
      else if (kd == 0)
        stage_chunk(1, 0, (g + 1) & 1);
      const int jmax = (int)(nk - c * CH < CH ? nk - c * CH : CH);
      const float* srows = sobs + (size_t)(g & 1) * CH * L.rs;
      if (live) GRP_PAIRS_DISPATCH(DCP, L, cat, GRP_PAIRS_CALL);
    }
    // (every row of KDE kd was staged before the walk's last barrier: s_bmax[kd] is complete)
    const KdeEst e = grp_estimate(K, kd, dc, du, nk, s_bmax[kd], xc, m, sp, sn, m != m, certified);
    if (kd == 0)
      est_l = e;
    else if (vw)
      A.scr[b * A.P + iw] = grp_emit(D, st, certified, est_l, e, grp_floor<DEFF>(A));
  }
}
#undef GRP_PAIRS_CALL

__device__ __forceinline__ AcqResult grp_empty_record(int32_t flags) {
  AcqResult r;
  r.index = -1;
  r.score = r.pdf_l = r.pdf_g = NAN;
  r.rel = 0.f;
  r.flags = flags;
  r.shortlist = 0;
  r.near = 0;
  return r;
}

template <bool DEFF, bool MASK>
__global__ __launch_bounds__(GRP_SEL_THREADS) void groups_select_kernel(GrpArgs A) {
  __shared__ ExactShared sh;
  __shared__ GrpView vw[2];
  __shared__ int32_t slist[GRP_SEL_THREADS];
  __shared__ int32_t swc[GRP_SEL_THREADS / 64];
  __shared__ uint32_t s_U;
  __shared__ int32_t s_st, s_of, s_first1, s_none, s_near;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t q = blockIdx.x, b = q / A.S;  // request q = b S + s of group b
  const int D = A.M.D;
  const int64_t C = A.C;
  if (wv == 0) {
    int dc, du;
    const int st0 = grp_classify(A.M, b, &dc, &du);
    if (lane == 0) s_st = st0;
  }
  if (tid == 0) {
    s_U = hbx_f2ord(INFINITY);
    s_of = 0;
    s_first1 = INT32_MAX;
    s_none = 0;
    s_near = 0;
  }
  __syncthreads();
  const int st = s_st;
  if constexpr (MASK) {
    if (A.want && A.want[q] == 0) {  // (uniform) the skipped record, with the group's bits as the dense call sets them
      if (tid == 0) {
        A.res[q] = grp_empty_record(HBX_ACQ_SKIPPED | ((st & GRP_NO_MODEL)      ? HBX_ACQ_NO_MODEL
                                                       : (st & GRP_UNSUPPORTED) ? HBX_ACQ_UNSUPPORTED
                                                                                : 0));
        atomicAdd(A.stats + 1, 1ull);
      }
      return;
    }
  }
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED)) {
    if (tid == 0) {
      A.res[q] = grp_empty_record((st & GRP_NO_MODEL) ? HBX_ACQ_NO_MODEL : HBX_ACQ_UNSUPPORTED);
      if constexpr (MASK) atomicAdd(A.stats + 0, 1ull);
    }
    return;
  }
  const int64_t s0 = A.M.seg_off[b], n = A.M.seg_off[b + 1] - s0;
  const double* Xs = A.M.X + s0 * D;
  const int64_t* rows_g = A.M.order + s0;
  const int64_t* rows_b = A.M.order + s0 + (n - A.M.n_bad[b]);
  if (tid < 2) vw[tid] = grp_view(A.M, b, tid);
  GScreen* scr = A.scr + q * C;
  const double* cand = A.cand + q * C * D;
  // pass 1: U = min shi over the certified candidates, the overflow rule, the first certain score 1
  {
    uint32_t u = hbx_f2ord(INFINITY);
    int of = 0, f1 = INT32_MAX, n1 = 0;
    for (int64_t i = tid; i < C; i += GRP_SEL_THREADS) {
      const GScreen g = scr[i];
      if (g.fl & GS_FORCE) continue;
      u = min(u, hbx_f2ord(g.shi));
      of |= (g.fl & GS_OF) ? 1 : 0;
      if (g.fl & GS_ONE) {
        f1 = min(f1, (int)i);
        ++n1;
      }
    }
    atomicMin(&s_U, u);
    if (of) atomicOr(&s_of, 1);
    if (n1) {
      atomicMin(&s_first1, f1);
      atomicAdd(&s_none, n1);
    }
  }
  __syncthreads();
  const bool all = (st & GRP_EXACT_ONLY) || s_of;
  const float U = hbx_ord2f(s_U);
  const int32_t first1 = s_first1;
  // pass 2: the shortlist in index order, 256 candidates at a time; each entry's exact pdfs by the whole block
  double best = INFINITY, bl = NAN, bg = NAN;
  int64_t bidx = -1;
  int32_t nshort = 0;
  for (int64_t c0 = 0; c0 < C; c0 += GRP_SEL_THREADS) {
    const int64_t i = c0 + tid;
    bool in = false;
    if (i < C) {
      const GScreen g = scr[i];
      in = all || (g.fl & GS_FORCE) || ((g.fl & GS_ONE) ? (int32_t)i == first1 : g.slo <= U);
    }
    const int tot = grp_compact(in, swc, slist);
    for (int p = 0; p < tot; ++p) {
      const int64_t ip = c0 + slist[p];
      double l, g;
      grp_exact_both(vw, D, cand + ip * D, Xs, rows_g, rows_b, &sh, &l, &g);
      if (tid == 0) {
        const double s = bohb_score(g, l, grp_floor<DEFF>(A).f);
        scr[ip].score = s;
        scr[ip].fl |= GS_DONE;
        if (s < best) {  // index order: strict '<' keeps the first index (bohb.py:149-152; NaN never wins)
          best = s;
          bidx = ip;
          bl = l;
          bg = g;
        }
      }
      __syncthreads();
    }
    nshort += tot;
  }
  // the near set: every re-scored candidate the winner cannot be told apart from by the bounds
  __shared__ double s_best, s_rb;
  __shared__ int64_t s_bidx;
  if (tid == 0) {
    s_best = best;
    s_bidx = bidx;
    s_rb = bidx >= 0 ? (double)scr[bidx].rel : 0.0;
  }
  __threadfence_block();
  __syncthreads();  // (also: thread 0's stores to scr are visible to the block)
  const double sb = s_best, rb = s_rb;
  const int64_t wi = s_bidx;
  if (wi >= 0) {
    int cnt = 0;
    for (int64_t i = tid; i < C; i += GRP_SEL_THREADS) {
      const GScreen g = scr[i];
      if (!(g.fl & GS_DONE)) continue;
      const double s = g.score;
      if (i == wi || near_best(s, (double)g.rel, sb, rb)) ++cnt;
    }
    if (cnt) atomicAdd(&s_near, cnt);
  }
  __syncthreads();
  if (tid == 0) {
    AcqResult r = grp_empty_record(all ? HBX_ACQ_OVERFLOW : 0);
    r.shortlist = nshort;
    int near = s_near;
    // the candidates left out as certain exact 1s tie with a winner whose score is 1
    if (wi >= 0 && !all && sb == 1.0 && s_none > 1) near += s_none - 1;
    r.near = near;
    r.rel = (float)rb;
    if (near > 1) r.flags |= HBX_ACQ_NEAR_TIE;
    if (wi >= 0) {
      r.index = wi;
      r.score = sb;
      r.pdf_l = bl;
      r.pdf_g = bg;
    }
    A.res[q] = r;
    if constexpr (MASK) {
      atomicAdd(A.stats + 0, 1ull);
      atomicAdd(A.stats + 3, (unsigned long long)nshort);
    }
  }
}

// C == 0: every record is the empty one; want (nullable): the skipped record for the unwanted requests
__global__ void groups_empty_kernel(AcqResult* res, int64_t B, const uint8_t* want) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) res[b] = grp_empty_record(want && want[b] == 0 ? HBX_ACQ_SKIPPED : 0);
}

// ------------------------------------------------------------------------------------------
// Grouped top-k (hbx_kde_acquire_groups_topk): the k best candidates of every group's pool, ranked exactly.
// Launch 1 is groups_screen_kernel as hbx_kde_acquire_groups launches it; launch 2 is groups_topk_kernel, one block
// per group, in place of groups_select_kernel:
//   bound      U_k = the k-th smallest shi over the certified candidates (no GS_FORCE; a GS_ONE candidate counts
//              with its interval [0, 0]); fewer than k of them: +inf.  A radix select over the hbx_f2ord keys' four
//              8-bit digits from the top: per digit an LDS histogram of the keys matching the digits chosen so far
//              (the group's slots re-read, so any C), a scan over its 256 bins, the digit that holds the rank.  Counts
//              are integers: no dependence on thread timing.
//   shortlist  in index order, 256 candidates at a time: everything if the group is exact-only or a GS_OF is
//              present; every GS_FORCE candidate; every certified candidate that is not GS_ONE with slo <= U_k; and,
//              only when 0 <= U_k, the first k GS_ONE candidates by index.
//   re-score   both fp64 pdfs of every shortlisted candidate by the whole block (exact_setup / exact_pdf, driven as
//              groups_select_kernel drives them), then bohb_score; the pdfs go to the group's spill in the workspace.
//   ranking    the running best-(k+1) of hbx_topk_rank.h over (score bits, index, index); its LDS arrays are the
//              launch's dynamic LDS, sized from k (grp_topk_cap), beside ExactShared.  An entry's pdfs and rel are not
//              carried through the merges: they stay in the spill / the screen slot and are read by index at the end.
//   result     header and records by ordinary vector stores; HBX_ACQ_NEAR_TIE as the single top-k sets it (adjacent
//              returned entries; the last one and the best re-scored one left out), and also when the last returned
//              entry scores exactly 1 while certain exact-1 candidates were left unlisted.
//
// Why the shortlist holds the whole top-k.  Every certified candidate's true ln score lies in its [slo, shi]; a
// GS_ONE candidate's true score is exactly 1 (ln 0).  With k certified candidates, at least k have shi <= U_k, so at
// least k true scores are <= U_k and the k-th smallest true score is <= U_k: every member of the true top-k, ties by
// index included, has a true score <= U_k, hence slo <= U_k -- or is uncertified, and those are all listed.  (Fewer
// than k certified: U_k = +inf, everything certified passes.)  The added step, for the certain exact 1s: they all
// have the same exact score, so among themselves they rank by index.  One that is preceded by k others of lower
// index is preceded by k candidates of a score not above its own and a lower index, so it cannot be among the first
// k of the order by (score, index): only the first k by index can be returned, and with U_k < 0 none can (k true
// scores are below 1).  The ranking itself is over exact scores only, so the shortlist decides cost, never the
// result.
struct GrpTopk {
  char* out;     // B result blocks of 16 + 40 k bytes
  double2* pdf;  // [B][C] {pdf_l, pdf_g} of the re-scored candidates: the per-group spill
  int32_t k, cap;
};

// entries of the ranking's LDS arrays for k: a power of two with k + 1 + GRP_SEL_THREADS <= cap
static int grp_topk_cap(int32_t k) {
  const int need = k + 1 + GRP_SEL_THREADS;
  return need <= 512 ? 512 : need <= 1024 ? 1024 : 2048;
}
static_assert(HBX_TOPK_MAX_K + 1 + GRP_SEL_THREADS <= 2048, "a chunk fits behind the kept entries after a merge");

template <bool DEFF>
__global__ __launch_bounds__(GRP_SEL_THREADS) void groups_topk_kernel(GrpArgs A, GrpTopk K) {
  constexpr int T = GRP_SEL_THREADS;
  extern __shared__ __align__(16) unsigned char s_dyn[];  // the ranking's arrays: cap x (u64, i32, i32)
  __shared__ ExactShared sh;
  __shared__ GrpView vw[2];
  __shared__ int32_t slist[T];
  __shared__ double s_l[T], s_g[T];
  __shared__ int32_t swc[T / 64], swo[T / 64];
  __shared__ uint32_t s_hist[256], s_wsum[T / 64];
  __shared__ uint32_t s_prefix, s_rank;
  __shared__ int32_t s_st, s_of, s_ncert, s_none;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const int D = A.M.D;
  const int64_t C = A.C;
  const int32_t k = K.k;
  TopkHead* head = (TopkHead*)(K.out + b * (int64_t)(sizeof(TopkHead) + sizeof(TopkRec) * (size_t)k));
  TopkRec* rec = (TopkRec*)(head + 1);
  if (wv == 0) {
    int dc, du;
    const int st0 = grp_classify(A.M, b, &dc, &du);
    if (lane == 0) s_st = st0;
  }
  if (tid == 0) {
    s_of = 0;
    s_ncert = 0;
    s_none = 0;
    s_prefix = 0u;
    s_rank = (uint32_t)k;
  }
  __syncthreads();
  const int st = s_st;
  if (st & (GRP_NO_MODEL | GRP_UNSUPPORTED)) {
    if (tid == 0) *head = TopkHead{0, 0, (st & GRP_NO_MODEL) ? HBX_ACQ_NO_MODEL : HBX_ACQ_UNSUPPORTED, k};
    return;
  }
  const int64_t s0 = A.M.seg_off[b], n = A.M.seg_off[b + 1] - s0;
  const double* Xs = A.M.X + s0 * D;
  const int64_t* rows_g = A.M.order + s0;
  const int64_t* rows_b = A.M.order + s0 + (n - A.M.n_bad[b]);
  if (tid < 2) vw[tid] = grp_view(A.M, b, tid);
  const GScreen* scr = A.scr + b * C;
  const double* cand = A.cand + b * C * D;
  double2* pdf = K.pdf + b * C;
  // pass 1: the certified candidates, the certain 1s among them, the overflow rule
  {
    int of = 0, nc = 0, n1 = 0;
    for (int64_t i = tid; i < C; i += T) {
      const uint32_t fl = scr[i].fl;
      if (fl & GS_FORCE) continue;
      ++nc;
      of |= (fl & GS_OF) ? 1 : 0;
      n1 += (fl & GS_ONE) ? 1 : 0;
    }
    if (of) atomicOr(&s_of, 1);
    if (nc) atomicAdd(&s_ncert, nc);
    if (n1) atomicAdd(&s_none, n1);
  }
  __syncthreads();
  const bool all = (st & GRP_EXACT_ONLY) || s_of;
  const int32_t none = s_none;
  // the bound: U_k by radix select over the keys of shi, the top digit first
  float U = INFINITY;
  if (!all && s_ncert >= k) {  // uniform
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
      s_hist[tid] = 0u;  // (T == 256 bins)
      __syncthreads();
      const uint32_t prefix = s_prefix, rank = s_rank;
      for (int64_t i = tid; i < C; i += T) {
        const GScreen g = scr[i];
        if (g.fl & GS_FORCE) continue;
        const uint32_t key = hbx_f2ord(g.shi);
        if (((key ^ prefix) & himask) == 0) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      const uint32_t c = s_hist[tid];
      uint32_t incl = c;  // inclusive scan over the 256 bins: within the wave, then the waves before
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      if (lane == 63) s_wsum[wv] = incl;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < T / 64; ++w) incl += w < wv ? s_wsum[w] : 0u;
      const uint32_t excl = incl - c;
      if (excl < rank && rank <= incl) {  // exactly one bin: the matching keys number >= rank
        s_prefix = prefix | ((uint32_t)tid << shift);
        s_rank = rank - excl;
      }
      __syncthreads();
    }
    U = hbx_ord2f(s_prefix);
  }
  static_assert(T == 256, "one thread per histogram bin");
  TopkRank<T> rank;
  rank.init((uint64_t*)s_dyn, (int32_t*)(s_dyn + 8 * (size_t)K.cap), (int32_t*)(s_dyn + 12 * (size_t)K.cap), swc, K.cap,
            k + 1);  // the k best and the best excluded one (the near-tie test's last pair)
  // pass 2: the shortlist in index order, 256 candidates at a time; each entry's exact pdfs by the whole block
  const bool ones_in = U >= 0.f;
  int32_t nshort = 0, ones_seen = 0;
  for (int64_t c0 = 0; c0 < C; c0 += T) {
    const int64_t i = c0 + tid;
    GScreen g;
    g.fl = GS_FORCE;
    g.slo = g.shi = NAN;
    const bool live = i < C;
    if (live) g = scr[i];
    const bool one = live && !(g.fl & GS_FORCE) && (g.fl & GS_ONE);
    const uint64_t bo = __ballot(one);
    if (lane == 0) swo[wv] = __popcll(bo);
    __syncthreads();
    int obefore = ones_seen, otot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
      obefore += w < wv ? swo[w] : 0;
      otot += swo[w];
    }
    ones_seen += otot;
    bool in = false;
    if (live) {
      if (all || (g.fl & GS_FORCE))
        in = true;
      else if (one)
        in = ones_in && obefore + (int)__popcll(bo & ((1ull << lane) - 1)) < k;  // the first k certain 1s by index
      else
        in = g.slo <= U;
    }
    const int tot = grp_compact(in, swc, slist);
    for (int p = 0; p < tot; ++p) {
      const int64_t ip = c0 + slist[p];
      // grp_exact_both's statements, kept apart in this kernel: through the function the call at config #5's shape
      // with k = 16 took 30.42 ms against 30.32 - 30.34 ms for this form and for the kernel before the header
      // (profiles/groups_shared/); groups_select_kernel measured the same either way and takes the function
      exact_setup(&vw[0], D, cand + ip * D, &sh);
      const double l = exact_pdf(Xs, D, rows_g, &vw[0], &sh);
      __syncthreads();
      exact_setup(&vw[1], D, cand + ip * D, &sh);
      const double gd = exact_pdf(Xs, D, rows_b, &vw[1], &sh);
      if (tid == 0) {
        s_l[p] = l;
        s_g[p] = gd;
      }
      __syncthreads();
    }
    // the chunk's re-scored entries, one per thread in index order: pdfs to the spill, the score to the ranking
    bool acc = false;
    uint64_t key = 0;
    int32_t idx = 0;
    if (tid < tot) {
      const double l = s_l[tid], gd = s_g[tid];
      idx = (int32_t)(c0 + slist[tid]);
      pdf[idx] = make_double2(l, gd);
      const double s = bohb_score(gd, l, grp_floor<DEFF>(A).f);
      if (s == s) {  // NaN scores are never returned
        key = (uint64_t)__double_as_longlong(s);
        acc = rank.enters(key, idx);
      }
    }
    rank.push(acc, key, idx, idx);  // (its last barrier: slist, s_l, s_g are free again)
    nshort += tot;
  }
  rank.finish();
  __threadfence_block();
  __syncthreads();  // (the spill's stores are visible to the block)
  const int nbest = rank.nb;
  const int nout = nbest < k ? nbest : k;
  // the ranked records; HBX_ACQ_NEAR_TIE: an entry and the next one (the last returned one's next is the best
  // excluded entry, position k) cannot be told apart by the re-score's error bounds
  bool near = false;
  for (int j = tid; j < nout; j += T) {
    const int32_t idx = rank.si[j];
    const double s = __longlong_as_double((long long)rank.sk[j]);
    const float r = scr[idx].rel;
    const double2 lg = pdf[idx];
    TopkRec o;
    o.index = idx;
    o.score = s;
    o.pdf_l = lg.x;
    o.pdf_g = lg.y;
    o.rel = r;
    o.pad = 0;
    rec[j] = o;
    if (j + 1 < nbest) {
      const double s2 = __longlong_as_double((long long)rank.sk[j + 1]);
      near = near || near_best(s2, (double)scr[rank.si[j + 1]].rel, s, (double)r);
    }
    // the certain 1s left unlisted tie with a last returned entry whose score is 1
    if (j == nout - 1 && s == 1.0 && !all && none > (ones_in ? (none < k ? none : k) : 0)) near = true;
  }
  const int any_near = __syncthreads_or(near);
  if (tid == 0)
    *head = TopkHead{nout, nshort, (all ? HBX_ACQ_OVERFLOW : 0) | (any_near ? HBX_ACQ_NEAR_TIE : 0), k};
}

__global__ void groups_topk_empty_kernel(char* out, int64_t B, int32_t k) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) *(TopkHead*)(out + b * (int64_t)(sizeof(TopkHead) + sizeof(TopkRec) * (size_t)k)) = TopkHead{0, 0, 0, k};
}

#define GRP_WS_HEAD 256

// Which screen a call runs -- the one rule.  One request per group is hbx_kde_acquire_groups' own case: the
// chunk-splitting screen, always.  Several requests flatten to tiles = ceil(S C / 64) tiles per group: from
// GRP_TILES_MIN tiles on the tile screen runs, below that the chunk-splitting screen over the flattened pool.
// Measured at config #5's shape: 2 tiles 10.7 ms against 9.1 ms for the chunk-splitting screen,
// 3 tiles 12.1 against 13.3 (one of the four waves without a tile, and still ahead), 4 tiles 13.7 against 17.7.
// HBX_GROUPS_SCREEN = 1 / 2 forces the chunk-splitting / the tile screen for S > 1 (tests, A/B); read on every call
// like the other switches.
#define GRP_TILES_MIN 3
static bool grp_tile_screen(int64_t S, int64_t tiles) {
  if (S == 1) return false;
  const char* e = getenv("HBX_GROUPS_SCREEN");
  const int v = e ? atoi(e) : 0;
  if (v == 1 || v == 2) return v == 2;
  return tiles >= GRP_TILES_MIN;
}

// the snapshot's floor: the kernels' constant instances (grp_floor)
static bool grp_floor_default(const ScoreFloor& F) { return F.f == HBX_PDF_FLOOR_DEFAULT; }

// One screen launch: the bucket's instance (grp_model picked the bucket from D alone)
template <bool TILES, bool MASK = false>
static void grp_launch_screen(GrpArgs& A, hipStream_t s) {
  const int nw = A.M.D <= 32 ? 4 : 2;  // waves of the bucket's instance
  A.slabs = (A.tiles + nw - 1) / nw;  // the tile screen: one tile per wave
  const dim3 grid((unsigned)(A.M.B * (TILES ? A.slabs : A.tiles)));  // <= B * S * C <= INT32_MAX
#define GRP_LAUNCH_F(DCP, DUP, NW, DT, DEFF)                                                                  \
  do {                                                                                                        \
    if (TILES)                                                                                                \
      hipLaunchKernelGGL((groups_tiles_kernel<DCP, DUP, NW, DT, DEFF, MASK>), grid, dim3(64 * NW), 0, s, A);  \
    else                                                                                                      \
      hipLaunchKernelGGL((groups_screen_kernel<DCP, DUP, NW, DT, DEFF, MASK>), grid, dim3(64 * NW), 0, s, A); \
  } while (0)
#define GRP_LAUNCH(DCP, DUP, NW, DT)       \
  do {                                     \
    if (grp_floor_default(A.F))            \
      GRP_LAUNCH_F(DCP, DUP, NW, DT, true); \
    else                                   \
      GRP_LAUNCH_F(DCP, DUP, NW, DT, false); \
  } while (0)
  GRP_BUCKET_LAUNCH(A.M.D, GRP_LAUNCH);
#undef GRP_LAUNCH
#undef GRP_LAUNCH_F
}

// the argument block of one call: the model, the pools, the screen slots behind the workspace's head
static GrpArgs grp_args(const GrpModel& M, const ScoreFloor& F, const double* cand, int64_t S, int64_t C, void* results,
                        void* workspace) {
  GrpArgs A;
  A.M = M;
  A.F = F;
  A.cand = cand;
  A.S = S;
  A.C = C;
  A.P = S * C;
  A.tiles = (int32_t)((A.P + 63) / 64);
  A.slabs = 0;
  A.scr = (GScreen*)((char*)workspace + GRP_WS_HEAD);
  A.res = (AcqResult*)results;
  A.want = nullptr;
  A.stats = nullptr;
  return A;
}

// hbx_kde_acquire_groups (S = 1) and hbx_kde_acquire_groups_batch: the checks, the screen, the select
// the score floor of an entry point's rules (NULL: the reference snapshot's); HBX_ERR_ARG out of range
static int grp_rules_floor(const char* who, const hbx_rules* rules, ScoreFloor* F) {
  const int rc = hbx_rules_check(who, rules);
  if (rc) return rc;
  *F = hbx_score_floor(rules ? rules->pdf_floor : HBX_PDF_FLOOR_DEFAULT);
  return HBX_OK;
}

// MASK: hbx_kde_acquire_groups_batch_m -- the same checks, the same choice of screen (from the dense S and tile count:
// the host does not see the mask), the kernels' masked instances, the counters in the workspace's head zeroed first
template <bool MASK = false>
static int grp_acquire(const char* who, const GrpModel& M, const hbx_rules* rules, const double* cand, int64_t S,
                       int64_t C, void* results, void* workspace, int64_t ws_bytes, void* stream,
                       const uint8_t* want = nullptr) {
  ScoreFloor F;
  if (const int rc = grp_rules_floor(who, rules, &F)) return rc;
  const int64_t B = M.B;
  if (const int rc = grp_check_dim(who, M.D)) return rc;
  if (B < 0 || S < 0 || C < 0)
    return hbx_fail(HBX_ERR_ARG, "%s: B=%lld S=%lld C=%lld", who, (long long)B, (long long)S, (long long)C);
  if (!grp_counts_ok(B, S, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * S * C = %lld * %lld * %lld exceeds int32", who, (long long)B, (long long)S,
                    (long long)C);
  if (B == 0 || S == 0) return HBX_OK;
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (results)", who);
  hipStream_t s = (hipStream_t)stream;
  if (C == 0) {  // nothing to score: every record is the empty one
    hipLaunchKernelGGL(groups_empty_kernel, dim3((unsigned)((B * S + 255) / 256)), dim3(256), 0, s, (AcqResult*)results,
                       B * S, want);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  if (grp_model_null(M) || !cand || !workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const int64_t need = hbx_kde_groups_batch_workspace_bytes(B, S, C, M.D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  if (((uintptr_t)workspace & 15) || ((uintptr_t)results & 7))
    return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte, results 8-byte aligned", who);
  GrpArgs A = grp_args(M, F, cand, S, C, results, workspace);
  if constexpr (MASK) {
    A.want = want;
    A.stats = (unsigned long long*)workspace;
    HBX_HIP(hipMemsetAsync(workspace, 0, 4 * sizeof(unsigned long long), s));
  }
  if (grp_tile_screen(S, A.tiles))
    grp_launch_screen<true, MASK>(A, s);
  else
    grp_launch_screen<false, MASK>(A, s);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL((grp_floor_default(F) ? groups_select_kernel<true, MASK> : groups_select_kernel<false, MASK>),
                     dim3((unsigned)(B * S)), dim3(GRP_SEL_THREADS), 0, s, A);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

// hbx_kde_acquire_groups_topk: grp_acquire's checks with S = 1, the same screen, groups_topk_kernel as the select
static int grp_acquire_topk(const char* who, const GrpModel& M, const hbx_rules* rules, const double* cand, int64_t C,
                            int32_t k, void* results, void* workspace, int64_t ws_bytes, void* stream) {
  ScoreFloor F;
  if (const int rc = grp_rules_floor(who, rules, &F)) return rc;
  const int64_t B = M.B;
  if (const int rc = grp_check_dim(who, M.D)) return rc;
  if (B < 0 || C < 0) return hbx_fail(HBX_ERR_ARG, "%s: B=%lld C=%lld", who, (long long)B, (long long)C);
  if (k < 1 || k > HBX_TOPK_MAX_K) return hbx_fail(HBX_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, HBX_TOPK_MAX_K);
  if (!grp_counts_ok(B, 1, C))
    return hbx_fail(HBX_ERR_ARG, "%s: B * C = %lld * %lld exceeds int32", who, (long long)B, (long long)C);
  if (B == 0) return HBX_OK;
  if (!results) return hbx_fail(HBX_ERR_ARG, "%s: null pointer (results)", who);
  if ((uintptr_t)results & 7) return hbx_fail(HBX_ERR_ARG, "%s: results must be 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  if (C == 0) {  // nothing to score: B headers with count 0
    hipLaunchKernelGGL(groups_topk_empty_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (char*)results, B,
                       k);
    HBX_LAUNCH_CHECK();
    return HBX_OK;
  }
  if (grp_model_null(M) || !cand || !workspace) return hbx_fail(HBX_ERR_ARG, "%s: null pointer", who);
  const int64_t need = hbx_kde_groups_topk_workspace_bytes(B, C, k, M.D);
  if (ws_bytes < need)
    return hbx_fail(HBX_ERR_ARG, "%s: workspace too small: %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
  if ((uintptr_t)workspace & 15) return hbx_fail(HBX_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
  GrpArgs A = grp_args(M, F, cand, 1, C, nullptr, workspace);
  GrpTopk K;
  K.out = (char*)results;
  K.pdf = (double2*)((char*)workspace + GRP_WS_HEAD + B * C * (int64_t)sizeof(GScreen));  // behind the screen slots
  K.k = k;
  K.cap = grp_topk_cap(k);
  grp_launch_screen<false>(A, s);
  HBX_LAUNCH_CHECK();
  hipLaunchKernelGGL(grp_floor_default(F) ? groups_topk_kernel<true> : groups_topk_kernel<false>, dim3((unsigned)B),
                     dim3(GRP_SEL_THREADS), (size_t)K.cap * 16, s, A, K);
  HBX_LAUNCH_CHECK();
  return HBX_OK;
}

extern "C" {

int64_t hbx_kde_groups_batch_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D) {
  if (D < 1 || D > HBX_MAX_D || !grp_counts_ok(B, S, C)) return -1;
  return GRP_WS_HEAD + B * S * C * (int64_t)sizeof(GScreen);
}

int64_t hbx_kde_groups_workspace_bytes(int64_t B, int64_t C, int32_t D) {
  return hbx_kde_groups_batch_workspace_bytes(B, 1, C, D);
}

int hbx_kde_acquire_groups(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                           const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                           const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                           const int32_t* nlev_bad, const double* cand, int64_t C, void* results, void* workspace,
                           int64_t ws_bytes, void* stream) {
  return grp_acquire("hbx_kde_acquire_groups",
                     grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad),
                     nullptr, cand, 1, C, results, workspace, ws_bytes, stream);
}

int hbx_kde_acquire_groups_batch(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                 const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                 const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                 const int32_t* nlev_bad, const double* cand, int64_t S, int64_t C, void* results,
                                 void* workspace, int64_t ws_bytes, void* stream) {
  return grp_acquire("hbx_kde_acquire_groups_batch",
                     grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad),
                     nullptr, cand, S, C, results, workspace, ws_bytes, stream);
}

int hbx_kde_acquire_groups_batch_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                   const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                   const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                   const int32_t* nlev_bad, const double* cand, int64_t S, int64_t C, void* results,
                                   void* workspace, int64_t ws_bytes, void* stream, const hbx_rules* rules) {
  return grp_acquire(rules ? "hbx_kde_acquire_groups_batch_r" : "hbx_kde_acquire_groups_batch",
                     grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad),
                     rules, cand, S, C, results, workspace, ws_bytes, stream);
}

int hbx_kde_acquire_groups_batch_m(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                   const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                   const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                   const int32_t* nlev_bad, const double* cand, int64_t S, int64_t C,
                                   const uint8_t* want, void* results, void* workspace, int64_t ws_bytes, void* stream,
                                   const hbx_rules* rules) {
  return grp_acquire<true>("hbx_kde_acquire_groups_batch_m",
                           grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good,
                                     nlev_bad),
                           rules, cand, S, C, results, workspace, ws_bytes, stream, want);
}

// the masked acquisition's counters (the workspace's head): synchronises the device
int hbx_kde_groups_request_stats(const void* workspace, int64_t* out4) {
  if (!workspace || !out4) return hbx_fail(HBX_ERR_ARG, "hbx_kde_groups_request_stats: null pointer");
  HBX_HIP(hipDeviceSynchronize());
  unsigned long long v[4];
  HBX_HIP(hipMemcpy(v, workspace, sizeof(v), hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k) out4[k] = (int64_t)v[k];
  return HBX_OK;
}

// the grouped workspace (the screen slots) followed by the re-scored candidates' pdfs, 16 bytes per candidate: the
// ranking's entries refer to them by index, so the spill does not grow with k
int64_t hbx_kde_groups_topk_workspace_bytes(int64_t B, int64_t C, int32_t k, int32_t D) {
  if (k < 1 || k > HBX_TOPK_MAX_K) return -1;
  const int64_t base = hbx_kde_groups_batch_workspace_bytes(B, 1, C, D);
  return base < 0 ? -1 : base + B * C * (int64_t)sizeof(double2);
}

int hbx_kde_acquire_groups_topk(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                const int32_t* nlev_bad, const double* cand, int64_t C, int32_t k, void* results,
                                void* workspace, int64_t ws_bytes, void* stream) {
  return grp_acquire_topk("hbx_kde_acquire_groups_topk",
                          grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad),
                          nullptr, cand, C, k, results, workspace, ws_bytes, stream);
}

int hbx_kde_acquire_groups_topk_r(const double* X, int32_t D, const int64_t* seg_off, int64_t B, const int64_t* order,
                                  const int64_t* n_good, const int64_t* n_bad, const int32_t* vartype,
                                  const double* bw_good, const double* bw_bad, const int32_t* nlev_good,
                                  const int32_t* nlev_bad, const double* cand, int64_t C, int32_t k, void* results,
                                  void* workspace, int64_t ws_bytes, void* stream, const hbx_rules* rules) {
  return grp_acquire_topk("hbx_kde_acquire_groups_topk_r",
                          grp_model(X, D, seg_off, B, order, n_good, n_bad, vartype, bw_good, bw_bad, nlev_good, nlev_bad),
                          rules, cand, C, k, results, workspace, ws_bytes, stream);
}

}  // extern "C"
