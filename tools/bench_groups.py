"""Grouped acquisition at config #5's shape: B = 1e4 brackets x n = 1e3 configs, 24 continuous + 8 categorical
dims (4 levels), C = 64 candidates per bracket (the reference's num_samples).

Times, with device events around REPS warmed repetitions each:
  acquire        hbx_kde_acquire_groups alone (candidates already on the device)
  sample+acquire hbx_kde_sample_groups + hbx_kde_acquire_groups
  chain          hbx_seg_argsort_ex + hbx_kde_fit + sample + acquire (promote's successor: refit all, propose all)
and the baseline the library offered before: per bracket kde.fit_pair_from_rows (two hbx_kde_prepare calls) +
KDEPair.acquire, on a subsample of SUB brackets (wall clock per bracket, synchronised), extrapolated to B --
reported with and without the prepare time.  The grouped picks are checked against the baseline's on the subsample.

    python tools/bench_groups.py [--B 10000] [--n 1000] [--C 64] [--reps 20] [--sub 200] [--out FILE]

Writes one JSON document (default profiles/groups/bench_groups.json) and prints it.

    python tools/bench_groups.py --requests S [--loop-only] [--out FILE]

times S get_config requests per bracket instead (requests_bench below): the batched call under each screen against S
one-request calls; prints one JSON line and writes it only where --out says.

    python tools/bench_groups.py --topk K [--out FILE]

times the k best candidates per bracket (topk_bench below): hbx_kde_acquire_groups_topk against the batched call with
S = K pools and the per-bracket acquire_topk loop; prints one JSON line and writes it only where --out says.

    python tools/bench_groups.py --logpdf [--out FILE]

times hbx_kde_logpdf_groups (logpdf_bench below) in default and FP64_ONLY mode at config #5's shape and at a plain
unsigned shape (8c) against the per-bracket prepare + logpdf loop; writes profiles/groups_logpdf/bench_groups_logpdf.json.

    python tools/bench_groups.py --get-config [--requests S] [--skip-random] [--counts K] [--no-parent] [--out FILE]

times the grouped get_config (get_config_bench below): hbx_kde_propose_groups against its parts and against
propose(requests=S) plus a host prior fill; writes profiles/groups_get_config/bench_groups_get_config.json.

    python tools/bench_groups.py --sh [--sh-max-budget 729] [--fills needed] [--out FILE]

times the grouped successive-halving transition (sh_bench below): hbx_sh_advance_groups alone against the sync-free
torch composition (stable argsort of the mask, gather, where), the two taking turns, and one full GroupHyperband
iteration with a device objective; writes profiles/groups_sh/bench_groups_sh.json.

    python tools/bench_groups.py --impute [--out FILE]

times the imputation of a conditional space's NaN entries (impute_bench below): hbx_kde_impute_groups, the fit on the
view and the whole refit against the plain refit on NaN-free data and against a plain gather of the same rows; writes
profiles/impute/bench_impute.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpbandster_amd import _native as N  # noqa: E402
from hpbandster_amd import groups, kde  # noqa: E402
from hpbandster_amd import synthetic as S  # noqa: E402

PEAK_FP32_TFLOPS = 157.3  # MI355X peak fp32 vector rate (bench.py's basis)
W = 92  # algorithmic flops per (candidate, observation) pair at 24c + 8u


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def sampler(gm, L, sh, lvd, seed, C, cands, derr):
    """The hbx_kde_sample_groups call of C candidates per bracket into ``cands`` / ``derr`` (counter base 0, stream
    id 0), its arguments taken once: the function a timed loop calls."""
    args = gm.model_args(groups.SAMPLE_ARGS) + (N.ptr(lvd), 3.0, seed, 0, 0, C, N.ptr(cands), N.ptr(derr), sh)

    def call():
        N.check(L.hbx_kde_sample_groups(*args))
    return call


def requests_bench(a, gm, L, sh, lvd):
    """--requests R: R pools of C candidates per bracket (one hbx_kde_sample_groups call with pool R C), then
      loop         R back-to-back hbx_kde_acquire_groups calls over the R request slices (--loop-only: nothing
                   else, so a library from before the batched call can be timed through HBX_LIB_PATH)
      batch        hbx_kde_acquire_groups_batch, the screen chosen by the library's rule
      batch_chunk  the same with HBX_GROUPS_SCREEN=1 (the chunk-splitting screen over the flattened pool)
      batch_tile   the same with HBX_GROUPS_SCREEN=2 (the tile screen)
    The loop reads request s of every bracket from its own contiguous [B, C, D] copy: the one-request call takes no
    stride.  Prints one JSON line; --out writes it too."""
    dev = gm.device
    B, R, C, D = gm.B, a.requests, a.C, gm.D
    pool = torch.empty((B, R * C, D), dtype=torch.float64, device=dev)
    derr = torch.empty((B, R * C), dtype=torch.uint8, device=dev)
    sampler(gm, L, sh, lvd, S.SEED_CAND, R * C, pool, derr)()
    cands = pool.view(B, R, C, D)
    model = gm.model_args()
    slices = [cands[:, s].contiguous() for s in range(R)]
    wsb1 = int(L.hbx_kde_groups_workspace_bytes(B, C, D))
    ws1 = torch.empty(wsb1, dtype=torch.uint8, device=dev)
    res1 = torch.empty((R, B, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)

    def loop():
        for s in range(R):
            N.check(L.hbx_kde_acquire_groups(*model, N.ptr(slices[s]), C, N.ptr(res1[s]), N.ptr(ws1), wsb1, sh))

    out = {"workload": "grouped_requests_b%d_n%d_d32_24c8u_s%d_c%d" % (B, a.n, R, C),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "requests": R,
           "library": N.LIB_PATH, "loop_ms": timed(loop, a.reps)}
    if not a.loop_only:
        wsb = int(L.hbx_kde_groups_batch_workspace_bytes(B, R, C, D))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        res = torch.empty((B, R, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)

        def batch():
            N.check(L.hbx_kde_acquire_groups_batch(*model, N.ptr(cands), R, C, N.ptr(res), N.ptr(ws), wsb, sh))

        for key, screen in (("batch_ms", None), ("batch_chunk_screen_ms", "1"), ("batch_tile_screen_ms", "2")):
            if screen is None:
                os.environ.pop("HBX_GROUPS_SCREEN", None)
            else:
                os.environ["HBX_GROUPS_SCREEN"] = screen
            out[key] = timed(batch, a.reps)
            picks = groups.GroupPicks.from_bytes(res.cpu().numpy().tobytes(), B, R)
            out[key.replace("_ms", "_mean_shortlist_per_request")] = float(picks.shortlist.mean())
        os.environ.pop("HBX_GROUPS_SCREEN", None)
        batch()
        picks = groups.GroupPicks.from_bytes(res.cpu().numpy().tobytes(), B, R)
        one = np.frombuffer(res1.cpu().numpy().tobytes(), dtype=groups.RECORD).reshape(R, B)
        agree = int(sum(np.array_equal(picks.index[:, s], one["index"][s]) and
                        np.array_equal(picks.score[:, s], one["score"][s], equal_nan=True) for s in range(R)))
        out.update({"workspace_bytes": wsb, "candidate_bytes": int(cands.numel()) * 8,
                    "picked": int((picks.index >= 0).sum()), "max_shortlist": int(picks.shortlist.max()),
                    "overflow_requests": int(((picks.flags & 1) != 0).sum()),
                    "near_tie_requests": int(((picks.flags & 2) != 0).sum()),
                    "requests_agreeing_with_loop": agree, "speedup_vs_loop": out["loop_ms"] / out["batch_ms"]})
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if a.loop_only or out["requests_agreeing_with_loop"] == R else 1


def topk_bench(a, gm, L, sh, lvd):
    """--topk K: K configurations per bracket out of one call.
      topk         hbx_kde_acquire_groups_topk over one pool of C candidates per bracket, k = K
      batch        hbx_kde_acquire_groups_batch with S = K pools per bracket: the device route to K picks per
                   bracket the library offered before (it screens K pools where the top-k screens one)
      acquire      hbx_kde_acquire_groups over the same pool (one pick: the screen both share plus its select)
      loop         per bracket kde.fit_pair_from_rows + KDEPair.acquire_topk on --sub subsampled brackets (wall
                   clock, synchronised), extrapolated to B; its ranked entries are compared with topk's
    and reports the shortlist per group (mean, maximum) and the share of groups flagged NEAR_TIE."""
    dev = gm.device
    B, K, C, D = gm.B, a.topk, a.C, gm.D
    model = gm.model_args()
    pool = torch.empty((B, K * C, D), dtype=torch.float64, device=dev)
    derr = torch.empty((B, K * C), dtype=torch.uint8, device=dev)
    sampler(gm, L, sh, lvd, S.SEED_CAND, K * C, pool, derr)()
    cands_s = pool.view(B, K, C, D)
    cands = cands_s[:, 0].contiguous()  # the top-k's one pool: request 0's
    step = kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * K
    wsk = int(L.hbx_kde_groups_topk_workspace_bytes(B, C, K, D))
    wsb = int(L.hbx_kde_groups_batch_workspace_bytes(B, K, C, D))
    ws1 = int(L.hbx_kde_groups_workspace_bytes(B, C, D))
    ws = torch.empty(max(wsk, wsb, ws1), dtype=torch.uint8, device=dev)
    res_k = torch.empty((B, step), dtype=torch.uint8, device=dev)
    res_s = torch.empty((B, K, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)
    res_1 = torch.empty((B, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)

    def topk():
        N.check(L.hbx_kde_acquire_groups_topk(*model, N.ptr(cands), C, K, N.ptr(res_k), N.ptr(ws), wsk, sh))

    def batch():
        N.check(L.hbx_kde_acquire_groups_batch(*model, N.ptr(cands_s), K, C, N.ptr(res_s), N.ptr(ws), wsb, sh))

    def acquire():
        N.check(L.hbx_kde_acquire_groups(*model, N.ptr(cands), C, N.ptr(res_1), N.ptr(ws), ws1, sh))

    ms_topk, ms_batch, ms_acq = timed(topk, a.reps), timed(batch, a.reps), timed(acquire, a.reps)
    picks = groups.GroupPicks.from_bytes(res_1.cpu().numpy().tobytes(), B)
    batch()
    picks_s = groups.GroupPicks.from_bytes(res_s.cpu().numpy().tobytes(), B, K)
    topk()
    top = groups.GroupTopK.from_bytes(res_k.cpu().numpy().tobytes(), B, K)
    first_ok = int(np.sum((top.index[:, 0] == picks.index) & (top.score[:, 0] == picks.score)))
    # the per-bracket loop on a subsample
    sub = np.unique(np.linspace(0, B - 1, min(a.sub, B)).astype(np.int64))
    ng, nb = int(gm.n_good[0]), int(gm.n_bad[0])
    bwg, bwb = gm.bandwidths()
    nlg, nlb = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    order_h = gm.order.cpu().numpy()
    seg = gm.seg_host
    vts = gm.var_type
    t_prep, t_acq, agree = [], [], 0
    for it, b in enumerate(np.concatenate([sub[:3], sub])):  # the first three again as warm-up
        s, e = int(seg[b]), int(seg[b + 1])
        Xb = gm.X[s:e].cpu().numpy()
        o = order_h[s:e]
        cb = cands[b]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pair = kde.fit_pair_from_rows(Xb, o[:ng], o[e - s - nb:], vts, bwg[b], bwb[b], nlg[b], nlb[b], device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = pair.acquire_topk(cb, K)
        t2 = time.perf_counter()
        if it >= 3:
            t_prep.append(t1 - t0)
            t_acq.append(t2 - t1)
            c = int(top.count[b])
            agree += int(r.count == c and np.array_equal(r.index, top.index[b, :c]) and
                         np.array_equal(r.score, top.score[b, :c]) and np.array_equal(r.pdf_l, top.pdf_l[b, :c]) and
                         np.array_equal(r.pdf_g, top.pdf_g[b, :c]))
    prep_ms, acq_ms = 1e3 * float(np.mean(t_prep)), 1e3 * float(np.mean(t_acq))
    out = {"workload": "grouped_topk_b%d_n%d_d32_24c8u_c%d_k%d" % (B, a.n, C, K),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "k": K, "library": N.LIB_PATH,
           "topk_ms": ms_topk, "batch_s_eq_k_ms": ms_batch, "acquire_one_pick_ms": ms_acq,
           "select_over_one_pick_ms": ms_topk - ms_acq,
           "mean_shortlist": float(top.shortlist.mean()), "max_shortlist": int(top.shortlist.max()),
           "one_pick_mean_shortlist": float(picks.shortlist.mean()),
           "batch_mean_shortlist_per_request": float(picks_s.shortlist.mean()),
           "returned_per_group_mean": float(top.count.mean()),
           "near_tie_share": float(((top.flags & 2) != 0).mean()),
           "overflow_groups": int(((top.flags & 1) != 0).sum()),
           "entry0_equals_one_pick": first_ok, "workspace_bytes": wsk,
           "loop": {"subsample": int(sub.size), "prepare_ms_per_group": prep_ms, "acquire_topk_ms_per_group": acq_ms,
                    "loop_ms_extrapolated": B * (prep_ms + acq_ms), "blocks_agree": agree},
           "speedup_vs_batch": ms_batch / ms_topk}
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if agree == sub.size and first_ok == B else 1


def _same_within(a, b, rtol):
    """a and b agree entry by entry: the same NaNs, finite values within rtol * max(1, |b|); -inf on one side against
    a finite log-space value on the other is accepted (the fp64 pdf underflowed to 0: either answer is in contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    rest = ~np.isnan(a) & ~fin
    if not np.all(np.isneginf(a[rest]) | np.isneginf(b[rest])):
        return False
    return bool(np.all(np.abs(a[fin] - b[fin]) <= rtol * np.maximum(1.0, np.abs(b[fin]))))


def logpdf_shape(a, dev, L, name, dc, du, lev):
    """One shape of --logpdf: B brackets of n rows, dc continuous + du categorical dims, C sampled candidates each."""
    B, n, C, D = a.B, a.n, a.C, dc + du
    vts = S.var_type_string(dc, du)
    losses = torch.from_numpy(S.make_bracket_losses(B, n).reshape(-1)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    X = torch.empty((B * n, D), dtype=torch.float64, device=dev)
    X[:, :dc] = torch.rand((B * n, dc), dtype=torch.float64, device=dev, generator=g)
    if du:
        X[:, dc:] = torch.randint(0, lev, (B * n, du), device=dev, generator=g).to(torch.float64)
    seg = np.arange(B + 1, dtype=np.int64) * n
    gm = groups.fit_groups(X, losses, seg, vts, device=dev)
    sh = N.stream_handle(None, dev)
    lvd = torch.tensor([0] * dc + [lev] * du, dtype=torch.int32, device=dev)
    cands = torch.empty((B, C, D), dtype=torch.float64, device=dev)
    derr = torch.empty((B, C), dtype=torch.uint8, device=dev)
    sampler(gm, L, sh, lvd, S.SEED_CAND, C, cands, derr)()
    model = gm.model_args()
    wsb = gm.workspace_bytes_logpdf(C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ll = torch.empty((B, C), dtype=torch.float64, device=dev)
    lg = torch.empty((B, C), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {"dims": "%dc+%du" % (dc, du), "n_good": int(gm.n_good[0]), "n_bad": int(gm.n_bad[0]), "workspace_bytes": wsb}
    host = {}
    for key, flags in (("default", 0), ("fp64_only", groups.LOGPDF_FP64_ONLY)):
        def call():
            N.check(L.hbx_kde_logpdf_groups(*model, N.ptr(cands), C, 1e-5, flags, N.ptr(ll), N.ptr(lg), N.ptr(status),
                                            N.ptr(ws), wsb, sh))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:  # every repetition between its own pair of device events
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        stats = np.zeros(4, dtype=np.int64)
        N.check(L.hbx_kde_logpdf_groups_stats(N.ptr(ws), stats.ctypes.data))
        out[key] = {"ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
                    "stats": [int(v) for v in stats], "fp32_share": float(stats[0]) / float(2 * B * C)}
        host[key] = (ll.cpu().numpy(), lg.cpu().numpy())
    st = status.cpu().numpy()
    out["groups_exact_l"] = int(((st & groups.GRP_EXACT_L) != 0).sum())
    out["groups_exact_g"] = int(((st & groups.GRP_EXACT_G) != 0).sum())
    out["modes_agree"] = bool(_same_within(host["default"][0], host["fp64_only"][0], 2e-5) and
                              _same_within(host["default"][1], host["fp64_only"][1], 2e-5))
    # the per-bracket loop on a subsample: what the library offered before
    sub = np.unique(np.linspace(0, B - 1, min(a.sub, B)).astype(np.int64))
    ng, nb = int(gm.n_good[0]), int(gm.n_bad[0])
    bwg, bwb = gm.bandwidths()
    nlg, nlb = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    order_h = gm.order.cpu().numpy()
    cands_h = cands.cpu().numpy()
    t_prep, t_lp, agree = [], [], 0
    for it, b in enumerate(np.concatenate([sub[:3], sub])):  # the first three again as warm-up
        s, e = int(seg[b]), int(seg[b + 1])
        Xb = gm.X[s:e].cpu().numpy()
        o = order_h[s:e]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pair = kde.fit_pair_from_rows(Xb, o[:ng], o[e - s - nb:], vts, bwg[b], bwb[b], nlg[b], nlb[b], device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        l1 = pair.good.logpdf(cands_h[b])
        g1 = pair.bad.logpdf(cands_h[b])
        t2 = time.perf_counter()
        if it >= 3:
            t_prep.append(t1 - t0)
            t_lp.append(t2 - t1)
            agree += int(_same_within(host["default"][0][b], l1, 2e-5) and _same_within(host["default"][1][b], g1, 2e-5))
    prep_ms, lp_ms, lp_min = 1e3 * float(np.mean(t_prep)), 1e3 * float(np.mean(t_lp)), 1e3 * float(np.min(t_lp))
    out["loop"] = {"subsample": int(sub.size), "prepare_ms_per_group": prep_ms, "logpdf_ms_per_group": lp_ms,
                   "logpdf_ms_per_group_fastest": lp_min, "loop_ms_extrapolated": B * (prep_ms + lp_ms),
                   "loop_ms_extrapolated_without_prepare": B * lp_ms,
                   "loop_ms_extrapolated_without_prepare_fastest": B * lp_min, "groups_agree": agree}
    slowest = max(out["default"]["ms_max"], out["fp64_only"]["ms_max"])
    out["slowest_grouped_vs_fastest_loop_without_prepare"] = B * lp_min / slowest
    out["default_not_slower_than_fp64_only"] = bool(out["default"]["ms_mean"] <= out["fp64_only"]["ms_mean"])
    return out, agree == sub.size and out["modes_agree"]


def logpdf_bench(a, dev, L):
    """--logpdf: hbx_kde_logpdf_groups at config #5's shape (24c + 8u, 4 levels) and at a plain unsigned shape (8c),
    same B, n, C.  Per shape: the grouped call in default and FP64_ONLY mode (device events around each of REPS warmed
    repetitions: mean, fastest, slowest), the four counters of each mode, and the only route the library offered
    before -- per bracket gm.pair(b)'s two hbx_kde_prepare calls plus good.logpdf and bad.logpdf, on --sub subsampled
    brackets (wall clock, synchronised), extrapolated to B with and without the prepare time, its values compared
    with the grouped call's.  Writes profiles/groups_logpdf/bench_groups_logpdf.json (or --out) and prints it."""
    a.out = a.out or os.path.join(ROOT, "profiles", "groups_logpdf", "bench_groups_logpdf.json")
    out = {"workload": "grouped_logpdf_b%d_n%d_c%d" % (a.B, a.n, a.C), "device": torch.cuda.get_device_name(0),
           "reps": a.reps, "rtol": 1e-5, "shapes": {}}
    ok = True
    for name, dc, du in (("config5_24c8u", 24, 8), ("plain_8c", 8, 0)):
        out["shapes"][name], good = logpdf_shape(a, dev, L, name, dc, du, 4)
        ok = ok and good
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if ok else 1


def each_timed(fn, reps, warm=3):
    """{mean, min, max} ms of fn, every warmed repetition between its own pair of device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return {"ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def get_config_bench(a, gm, L, sh, lvd, levels):
    """--get-config: S = --requests get_config requests per bracket, every one answered with a configuration.
      fused      hbx_kde_propose_groups (records kept, pools left in the workspace)
      two_calls  hbx_kde_sample_groups (pool S C) + hbx_kde_acquire_groups_batch: the composition's first two calls
      finish     hbx_kde_finish_groups alone, over the pools and records the two calls left
      parent     what the library offered before for the same answer: propose(requests=S) -- the same two calls, the
                 records fetched, the winning rows gathered through the host -- plus a numpy prior fill of the rows
                 the random fraction takes and of the NaN rows (wall clock, synchronised)
    The fused call's rows and sources are compared with finish's over the two calls' outputs (byte equality).
    --skip-random adds fused_skip_random: hbx_kde_propose_groups_m with HBX_PROPOSE_SKIP_RANDOM (requests the random
    fraction takes are not sampled and scored; rows and sources compared with the fused call's, byte for byte).
    --counts K adds fused_counts: hbx_kde_propose_groups_m under the mask of a deficit of K requests in every 100th
    run and none elsewhere (a crashed worker's fill call), the wanted rows compared with the fused call's.  Both print
    their line beside the fused call's, with hbx_kde_groups_request_stats' counters."""
    dev = gm.device
    B, R, C, D = gm.B, a.requests, a.C, gm.D
    rf, seed = 1.0 / 3, S.SEED_CAND
    a.out = a.out or os.path.join(ROOT, "profiles", "groups_get_config", "bench_groups_get_config.json")
    model = gm.model_args()
    wsf = int(L.hbx_kde_propose_groups_workspace_bytes(B, R, C, D))
    wsb = int(L.hbx_kde_groups_batch_workspace_bytes(B, R, C, D))
    ws = torch.empty(wsf, dtype=torch.uint8, device=dev)
    pool = torch.empty((B, R, C, D), dtype=torch.float64, device=dev)
    derr = torch.empty((B, R, C), dtype=torch.uint8, device=dev)
    rec = torch.empty((B, R, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)
    rec_f = torch.empty_like(rec)
    rows, src = (torch.empty((B, R, D), dtype=torch.float64, device=dev),
                 torch.empty((B, R), dtype=torch.uint8, device=dev))
    rows_f, src_f = torch.empty_like(rows), torch.empty_like(src)

    def fused():
        N.check(L.hbx_kde_propose_groups(*model, N.ptr(lvd), 3.0, rf, seed, 0, 0, R, C, N.ptr(rows_f), N.ptr(src_f),
                                         N.ptr(rec_f), None, N.ptr(ws), wsf, sh))

    sample = sampler(gm, L, sh, lvd, seed, R * C, pool, derr)

    def two_calls():
        sample()
        N.check(L.hbx_kde_acquire_groups_batch(*model, N.ptr(pool), R, C, N.ptr(rec), N.ptr(ws), wsb, sh))

    def finish():
        N.check(L.hbx_kde_finish_groups(N.ptr(rec), N.ptr(pool), N.ptr(derr), N.ptr(lvd), D, B, R, C, rf, seed, 0, 0,
                                        N.ptr(rows), N.ptr(src), sh))

    lv = np.asarray(levels)

    def parent():
        got, picks = gm.propose(C, seed, levels, requests=R)
        rs = np.random.RandomState(0)
        fill = (rs.rand(B, R) < rf) | np.isnan(got).any(axis=2)
        draw = rs.rand(int(fill.sum()), D)
        cat = lv > 0
        draw[:, cat] = np.floor(draw[:, cat] * lv[cat])
        got[fill] = draw
        return got

    wsm = int(L.hbx_kde_propose_groups_m_workspace_bytes(B, R, C, D))
    ws_m = torch.empty(wsm, dtype=torch.uint8, device=dev)
    rows_m, src_m, rec_m = torch.empty_like(rows), torch.empty_like(src), torch.empty_like(rec)

    def masked(want, flags):
        def call():
            N.check(L.hbx_kde_propose_groups_m(*model, N.ptr(lvd), 3.0, rf, seed, 0, 0, R, C, N.ptr(want), flags,
                                               N.ptr(rows_m), N.ptr(src_m), N.ptr(rec_m), None, N.ptr(ws_m), wsm, sh,
                                               None))
        return call

    def request_stats():
        st = np.zeros(4, dtype=np.int64)
        N.check(L.hbx_kde_groups_request_stats(N.ptr(ws_m), st.ctypes.data))
        return dict(zip(("answered", "skipped", "screened_candidates", "rescored_candidates"), (int(v) for v in st)))

    out = {"workload": "grouped_get_config_b%d_n%d_d32_24c8u_s%d_c%d" % (B, a.n, R, C),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "requests": R, "random_fraction": rf,
           "workspace_bytes": wsf}
    two_calls()
    out["two_calls"] = each_timed(two_calls, a.reps)
    out["finish"] = each_timed(finish, a.reps)
    out["fused"] = each_timed(fused, a.reps)
    out["two_calls_then_finish"] = each_timed(lambda: (two_calls(), finish()), a.reps)
    same_m = True
    if a.skip_random:
        call = masked(None, groups.PROPOSE_SKIP_RANDOM)
        out["fused_skip_random"] = each_timed(call, a.reps)
        out["fused_skip_random"]["stats"] = request_stats()
        same_m = same_m and bool(torch.equal(rows_m.view(torch.int64), rows_f.view(torch.int64)) and
                                 torch.equal(src_m, src_f))
        print("fused             ", json.dumps(out["fused"], sort_keys=True))
        print("fused_skip_random ", json.dumps(out["fused_skip_random"], sort_keys=True))
    if a.counts:
        cnt = torch.zeros(B, dtype=torch.int64, device=dev)
        cnt[::100] = min(a.counts, R)
        want = groups.counts_to_mask(cnt, R).contiguous()
        call = masked(want, 0)
        out["fused_counts"] = each_timed(call, a.reps)
        out["fused_counts"].update(stats=request_stats(), counts=int(min(a.counts, R)), every=100)
        on = want.bool()
        same_m = same_m and bool(torch.equal(rows_m.view(torch.int64)[on], rows_f.view(torch.int64)[on]) and
                                 torch.equal(src_m[on], src_f[on]) and bool((src_m[~on] == 5).all()))
        print("fused             ", json.dumps(out["fused"], sort_keys=True))
        print("fused_counts      ", json.dumps(out["fused_counts"], sort_keys=True))
    out["masked_equals_fused"] = same_m
    t = []
    for it in range(0 if a.no_parent else 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parent()
        t.append(1e3 * (time.perf_counter() - t0))
    t = t or [float("nan")] * 5  # (--no-parent)
    out["parent_propose_plus_host_fill"] = {"ms_mean": float(np.mean(t[2:])), "ms_min": float(np.min(t[2:])),
                                            "ms_max": float(np.max(t[2:]))}
    same = bool(torch.equal(rows.view(torch.int64), rows_f.view(torch.int64)) and torch.equal(src, src_f) and
                torch.equal(rec, rec_f))
    sh_ = src_f.cpu().numpy()
    out.update({"fused_equals_composition": same,
                "sources": {str(k): int((sh_ == k).sum()) for k in range(5)},
                "finish_bytes_read": B * R * (48 + C), "finish_bytes_written": B * R * (8 * D + 1),
                "fused_slowest_minus_parts_fastest_ms": out["fused"]["ms_max"] - out["two_calls"]["ms_min"] -
                out["finish"]["ms_min"],
                "fused_mean_minus_parts_mean_ms": out["fused"]["ms_mean"] - out["two_calls"]["ms_mean"] -
                out["finish"]["ms_mean"],
                "parent_fastest_over_fused_slowest": out["parent_propose_plus_host_fill"]["ms_min"] /
                out["fused"]["ms_max"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if same and same_m else 1


def _torch_advance(X3, m, K, fresh):
    """The sync-free composition torch offers without hbx_sh_advance_groups: a stable argsort of the cleared mask per
    run, its first K, a gather, and a where for the fills (NaN rows without ``fresh``).  (rows, src, counts)."""
    B, n, D = X3.shape
    order = torch.argsort((m == 0).to(torch.uint8), dim=1, stable=True)[:, :K]
    got = X3.gather(1, order[:, :, None].expand(B, K, D))
    cnt = m.ne(0).sum(dim=1)
    j = torch.arange(K, device=X3.device)[None, :]
    keep = j < cnt[:, None]
    fi = (j - cnt[:, None]).clamp(min=0)
    if fresh is None:
        rows = torch.where(keep[:, :, None], got, torch.full_like(got, float("nan")))
        src = torch.where(keep, order, torch.full_like(order, -2 ** 31))
        nf = torch.zeros_like(cnt)
    else:
        rows = torch.where(keep[:, :, None], got, fresh.gather(1, fi[:, :, None].expand(B, K, D)))
        src = torch.where(keep, order, -1 - fi)
        nf = (K - cnt).clamp(min=0)
    return rows, src.to(torch.int32), torch.stack((cnt, nf), dim=1)


def _alternate(fns, reps, warm=3):
    """name -> {ms_mean, ms_min, ms_max}: the functions take turns, every call between its own pair of device events"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
        out[k] = {"ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}
    return out


def sh_bench(a, dev, L):
    """--sh: the stage transition of B runs.  hbx_sh_advance_groups alone at config #5's shape (n configurations per
    run, K = n // 3 survivors, D = 32) against the torch composition above, the two taking turns: without fills, with
    1 % crashed runs (and the fills offered), and with 1 % of the runs crashed whole (their stage all fills).  Then one
    full GroupHyperband iteration (eta = 3, budgets 1 .. --sh-max-budget) with a device objective: the synchronised
    wall time beside the device time of its calls."""
    from hpbandster_amd import promote
    B, n, D = a.B, a.n, 32
    K = n // 3
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    X = torch.rand((B * n, D), dtype=torch.float64, device=dev, generator=g)
    fresh = torch.rand((B, K, D), dtype=torch.float64, device=dev, generator=g)
    seg = np.arange(B + 1, dtype=np.int64) * n
    seg_d = torch.from_numpy(seg).to(dev)
    base_losses = torch.from_numpy(S.make_bracket_losses(B, n).reshape(-1)).to(dev)
    kk = np.full(B, float(K))
    moved = B * (n + K * 4 + 16) + 2 * B * K * D * 8  # mask in, src and counts out, K rows per run in and out
    out = {"shape": {"B": B, "n": n, "K": K, "D": D}, "reps": a.reps, "bytes": moved, "cases": {}}
    ok = True
    for name in ("no_fills", "crashed_runs_1pct", "crashed_brackets_1pct"):
        losses = base_losses.clone()
        if name == "crashed_runs_1pct":
            losses[torch.rand(B * n, device=dev, generator=g) < 0.01] = float("inf")
        elif name == "crashed_brackets_1pct":
            losses.view(B, n)[torch.rand(B, device=dev, generator=g) < 0.01] = float("inf")
        mask, nadv = promote.promote_segments(losses, seg, kk, device=dev, on_device=True)
        fr = None if name == "no_fills" else fresh
        bufs = (torch.empty((B, K, D), dtype=torch.float64, device=dev),
                torch.empty((B, K), dtype=torch.int32, device=dev), torch.zeros((B, 2), dtype=torch.int64, device=dev))
        frp, F = (N.ptr(fr), K) if fr is not None else (None, 0)

        def new():
            N.check(L.hbx_sh_advance_groups(N.ptr(X), D, N.ptr(seg_d), B, N.ptr(mask), frp, F, K, N.ptr(bufs[0]),
                                            N.ptr(bufs[1]), N.ptr(bufs[2]), N.stream_handle(None, dev)))

        def composition():
            return _torch_advance(X.view(B, n, D), mask.view(B, n), K, fr)

        new()
        want = composition()
        same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                               y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(bufs, want))
        del want
        t = _alternate({"new": new, "torch": composition}, a.reps)
        gbs = moved / (t["new"]["ms_mean"] * 1e-3) / 1e9
        out["cases"][name] = {
            "new": t["new"], "torch": t["torch"], "equal_outputs": bool(same),
            "deficit_runs": int((nadv < K).sum()), "new_gb_s": gbs, "new_fraction_of_8tb_s": gbs / 8000.0,
            "new_fraction_of_5p5tb_s": gbs / 5500.0, "speedup_mean": t["torch"]["ms_mean"] / t["new"]["ms_mean"],
            "new_slowest_below_torch_fastest": bool(t["new"]["ms_max"] < t["torch"]["ms_min"])}
        ok = ok and same and t["new"]["ms_max"] < t["torch"]["ms_min"]
    del X, fresh

    # one Hyperband iteration of B runs: ladder [ns], a device objective, every call between device events
    dc, du, lev = 24, 8, 4
    opt = groups.GroupBOHB(B, S.var_type_string(dc, du), [0] * dc + [lev] * du, num_samples=a.C, seed=4, device=dev)
    kw = dict(fills=a.fills) if a.fills != "all" else {}  # ('needed': only the deficits' fill requests are computed)
    hb = groups.GroupHyperband(opt, eta=3, min_budget=1, max_budget=a.sh_max_budget, **kw)
    ev = {}

    def stamped(name, fn):
        def f(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            ev.setdefault(name, []).append((e0, e1))
            return r
        return f

    def objective(rows, budget, info):
        return ((rows[..., 0] - 0.3) ** 2 + (rows[..., 1] - 0.7) ** 2 + 0.1 * rows[..., -1]) / budget

    opt.new_results = stamped("new_results", opt.new_results)
    opt.get_configs = stamped("get_configs", opt.get_configs)
    promote_plain, advance_plain = promote.promote_segments, groups.advance
    promote.promote_segments = stamped("promote", promote_plain)
    groups.advance = stamped("advance", advance_plain)
    runs = []
    try:
        for it in range(2):  # iteration 0 twice (the ladder's longest); the first run warms every shape
            hb.iterations = 0
            opt.configs, opt.losses, opt.kde_models, opt.counter = {}, {}, {}, 0
            ev.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hb.run(1, stamped("objective", objective), keep=None)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            calls = {k: float(sum(e0.elapsed_time(e1) for e0, e1 in v)) for k, v in ev.items()}
            runs.append({"wall_ms": wall, "calls_ms": calls, "calls_sum_ms": float(sum(calls.values()))})
    finally:
        promote.promote_segments, groups.advance = promote_plain, advance_plain
    out["hyperband_iteration"] = {"ladder": hb.ladder(0)[0], "budgets": hb.ladder(0)[1], "warm": runs[0],
                                  "timed": runs[1]}
    out["ok"] = bool(ok)
    a.out = a.out or os.path.join(ROOT, "profiles", "groups_sh", "bench_groups_sh.json")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if ok else 1


def impute_bench(a, dev, L):
    """--impute: conditional search spaces at config #5's shape.  8 of the 32 dims conditional (6 continuous, 2
    categorical, spread over the row), ~30 % of their entries NaN.  Times hbx_kde_impute_groups alone, the fit on the
    view, and argsort + impute + fit, against argsort + fit on NaN-free data of the same shape (the plain
    fit_groups) -- and a plain device gather of the same rows (torch.index_select), the rate the impute call is
    measured against: both read every view row's source once and write the view once."""
    B, n, dc, du, lev = a.B, a.n, 24, 8, 4
    D = dc + du
    vts = S.var_type_string(dc, du)
    levels = np.array([0] * dc + [lev] * du, dtype=np.int32)
    cond_dims = [1, 5, 9, 13, 17, 21, 25, 29]
    losses = torch.from_numpy(S.make_bracket_losses(B, n).reshape(-1)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    X = torch.empty((B * n, D), dtype=torch.float64, device=dev)
    X[:, :dc] = torch.rand((B * n, dc), dtype=torch.float64, device=dev, generator=g)
    X[:, dc:] = torch.randint(0, lev, (B * n, du), device=dev, generator=g).to(torch.float64)
    seg = np.arange(B + 1, dtype=np.int64) * n
    plain = groups.fit_groups(X, losses, seg, vts, device=dev)
    Xn = X.clone()
    for d in cond_dims:
        Xn[torch.rand(B * n, device=dev, generator=g) < 0.3, d] = float("nan")
    gm = groups.fit_groups(Xn, losses, seg, vts, device=dev, impute_seed=1, levels=levels)
    sh = N.stream_handle(None, dev)
    Nv = int(gm.seg_host[-1])
    lvd = torch.from_numpy(levels).to(dev)
    wb = int(L.hbx_kde_impute_groups_workspace_bytes(Nv, B, D))
    iws = torch.empty(wb, dtype=torch.uint8, device=dev)
    sb = int(L.hbx_sort_scratch_bytes(B * n))
    scr = torch.empty(sb, dtype=torch.uint8, device=dev)

    def argsort(m, order):
        N.check(L.hbx_seg_argsort_ex(N.ptr(m.losses), N.ptr(order_seg(m)), B, n, B * n, N.ptr(order), N.ptr(scr), sb,
                                     N.ORDER_NUMPY, sh))

    def order_seg(m):
        return getattr(m, "raw_seg_off", m.seg_off)

    def fit(m):
        N.check(L.hbx_kde_fit(N.ptr(m.X), D, N.ptr(m.seg_off), B, N.ptr(m.order), N.ptr(m.n_good_dev),
                              N.ptr(m.n_bad_dev), N.ptr(m.fac_good_dev), N.ptr(m.fac_bad_dev), N.ptr(m.vt_dev),
                              N.ptr(m.bw_good), N.ptr(m.bw_bad), N.ptr(m.nlev_good), N.ptr(m.nlev_bad), sh))

    def impute(m=gm):
        N.check(L.hbx_kde_impute_groups(N.ptr(m.raw_X), D, N.ptr(m.raw_seg_off), B, N.ptr(m.raw_order),
                                        N.ptr(m.n_good_dev), N.ptr(m.n_bad_dev), N.ptr(lvd), N.ptr(m.seg_off), Nv, 1,
                                        0, 0, N.ptr(m.X), N.ptr(m.order), N.ptr(m.src_rows),
                                        N.ptr(m.impute_counts), N.ptr(iws), wb, sh))

    # the same rows through a plain gather: global source row of every view row
    seg_d = torch.from_numpy(seg[:-1]).to(dev)
    rows = (gm.src_rows[:Nv].long() + seg_d.repeat_interleave(torch.from_numpy(np.diff(gm.seg_host)).to(dev)))
    out = torch.empty_like(gm.X)
    ms_impute = timed(impute, a.reps)
    ms_gather = timed(lambda: torch.index_select(gm.raw_X, 0, rows, out=out), a.reps)
    ms_fit_view = timed(lambda: fit(gm), a.reps)
    ms_chain = timed(lambda: (argsort(gm, gm.raw_order), impute(), fit(gm)), a.reps)
    ms_plain = timed(lambda: (argsort(plain, plain.order), fit(plain)), a.reps)
    ms_plain_fit = timed(lambda: fit(plain), a.reps)
    del out
    clean = groups.fit_groups(X, losses, seg, vts, device=dev, impute_seed=1, levels=levels)  # nothing to fill
    ms_clean = timed(lambda: impute(clean), a.reps)
    counts = gm.impute_counts.cpu().numpy()
    moved = 2.0 * Nv * D * 8
    res = {
        "workload": "impute_groups_b%d_n%d_d32_24c8u_8cond_30pct" % (B, n),
        "device": torch.cuda.get_device_name(0), "reps": a.reps, "view_rows": Nv,
        "n_good": int(gm.n_good[0]), "n_bad": int(gm.n_bad[0]),
        "nan_entries_filled": int(counts[:, 0].sum()), "prior_entries_filled": int(counts[:, 1].sum()),
        "impute_ms": ms_impute, "impute_nan_free_ms": ms_clean, "gather_ms": ms_gather, "bytes_moved": moved,
        "impute_gb_per_s": moved / ms_impute / 1e6, "gather_gb_per_s": moved / ms_gather / 1e6,
        "fraction_of_gather_rate": ms_gather / ms_impute,
        "fit_on_view_ms": ms_fit_view, "argsort_impute_fit_ms": ms_chain,
        "plain_fit_ms": ms_plain_fit, "plain_argsort_fit_ms": ms_plain,
        "workspace_bytes": wb,
    }
    a.out = a.out or os.path.join(ROOT, "profiles", "impute", "bench_impute.json")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--impute", action="store_true",
                    help="conditional spaces: the impute call and the fit on the view (impute_bench)")
    ap.add_argument("--sh", action="store_true", help="the grouped successive-halving transition (sh_bench)")
    ap.add_argument("--sh-max-budget", type=float, default=729.0,
                    help="--sh: the Hyperband iteration's budgets run from 1 to this (eta = 3)")
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sub", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--requests", type=int, default=1, help="S get_config requests per bracket (requests_bench)")
    ap.add_argument("--loop-only", action="store_true",
                    help="time only the S one-request calls (what a library without the batched call offers)")
    ap.add_argument("--topk", type=int, default=0, help="the K best candidates per bracket (topk_bench)")
    ap.add_argument("--logpdf", action="store_true", help="both KDEs' ln pdf of every pool (logpdf_bench)")
    ap.add_argument("--get-config", action="store_true",
                    help="a configuration per request with the reference's fall-backs (get_config_bench)")
    ap.add_argument("--skip-random", action="store_true",
                    help="--get-config: also the masked call that does not sample and score random requests")
    ap.add_argument("--counts", type=int, default=0,
                    help="--get-config: also the masked call with a deficit of K requests in every 100th run")
    ap.add_argument("--no-parent", action="store_true",
                    help="--get-config: leave out the host-side 'parent' composition (wall clock, seconds per call)")
    ap.add_argument("--fills", choices=("all", "needed"), default="all",
                    help="--sh: GroupSuccessiveHalving's fills option for the driven run")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    L = N.lib()
    if a.logpdf:
        return logpdf_bench(a, dev, L)
    if a.impute:
        return impute_bench(a, dev, L)
    if a.sh:
        return sh_bench(a, dev, L)
    B, n, C, dc, du, lev = a.B, a.n, a.C, 24, 8, 4
    D = dc + du
    vts = S.var_type_string(dc, du)
    levels = [0] * dc + [lev] * du
    # config #5's inputs as bench.py builds them: synthetic.py's losses, observations drawn on the device
    losses = torch.from_numpy(S.make_bracket_losses(B, n).reshape(-1)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    X = torch.empty((B * n, D), dtype=torch.float64, device=dev)
    X[:, :dc] = torch.rand((B * n, dc), dtype=torch.float64, device=dev, generator=g)
    X[:, dc:] = torch.randint(0, lev, (B * n, du), device=dev, generator=g).to(torch.float64)
    seg = np.arange(B + 1, dtype=np.int64) * n
    gm = groups.fit_groups(X, losses, seg, vts, device=dev)
    sh = N.stream_handle(None, dev)
    if a.get_config:
        return get_config_bench(a, gm, L, sh, torch.tensor(levels, dtype=torch.int32, device=dev), levels)
    if a.topk:
        return topk_bench(a, gm, L, sh, torch.tensor(levels, dtype=torch.int32, device=dev))
    if a.requests > 1 or a.loop_only:
        return requests_bench(a, gm, L, sh, torch.tensor(levels, dtype=torch.int32, device=dev))
    a.out = a.out or os.path.join(ROOT, "profiles", "groups", "bench_groups.json")
    cands = torch.empty((B, C, D), dtype=torch.float64, device=dev)
    derr = torch.empty((B, C), dtype=torch.uint8, device=dev)
    lvd = torch.tensor(levels, dtype=torch.int32, device=dev)
    wsb = gm.workspace_bytes(C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    res = torch.empty((B, kde.RESULT_BYTES), dtype=torch.uint8, device=dev)
    sb = int(L.hbx_sort_scratch_bytes(B * n))
    scr = torch.empty(sb, dtype=torch.uint8, device=dev)

    def refit():
        N.check(L.hbx_seg_argsort_ex(N.ptr(gm.losses), N.ptr(gm.seg_off), B, n, B * n, N.ptr(gm.order), N.ptr(scr), sb,
                                     N.ORDER_NUMPY, sh))
        N.check(L.hbx_kde_fit(N.ptr(gm.X), D, N.ptr(gm.seg_off), B, N.ptr(gm.order), N.ptr(gm.n_good_dev),
                              N.ptr(gm.n_bad_dev), N.ptr(gm.fac_good_dev), N.ptr(gm.fac_bad_dev), N.ptr(gm.vt_dev),
                              N.ptr(gm.bw_good), N.ptr(gm.bw_bad), N.ptr(gm.nlev_good), N.ptr(gm.nlev_bad), sh))

    sample = sampler(gm, L, sh, lvd, S.SEED_CAND, C, cands, derr)
    model = gm.model_args()

    def acquire():
        N.check(L.hbx_kde_acquire_groups(*model, N.ptr(cands), C, N.ptr(res), N.ptr(ws), wsb, sh))

    sample()
    ms_acq = timed(acquire, a.reps)
    ms_sa = timed(lambda: (sample(), acquire()), a.reps)
    ms_chain = timed(lambda: (refit(), sample(), acquire()), a.reps)
    ms_fit = timed(refit, a.reps)
    picks = groups.GroupPicks.from_bytes(res.cpu().numpy().tobytes(), B)
    ng, nb = int(gm.n_good[0]), int(gm.n_bad[0])
    pairs = float(B) * C * (ng + nb)
    rate = pairs / (ms_acq * 1e-3)

    # the per-bracket loop on a subsample
    sub = np.unique(np.linspace(0, B - 1, min(a.sub, B)).astype(np.int64))
    bwg, bwb = gm.bandwidths()
    nlg, nlb = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    order_h = gm.order.cpu().numpy()
    t_prep, t_acq, agree = [], [], 0
    for it, b in enumerate(np.concatenate([sub[:3], sub])):  # the first three again as warm-up
        s, e = int(seg[b]), int(seg[b + 1])
        Xb = gm.X[s:e].cpu().numpy()
        o = order_h[s:e]
        cb = cands[b]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pair = kde.fit_pair_from_rows(Xb, o[:ng], o[e - s - nb:], vts, bwg[b], bwb[b], nlg[b], nlb[b], device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = pair.acquire(cb)
        t2 = time.perf_counter()
        if it >= 3:
            t_prep.append(t1 - t0)
            t_acq.append(t2 - t1)
            agree += int(r.index == picks.index[b] and r.score == picks.score[b])
    prep_ms, acq_ms = 1e3 * float(np.mean(t_prep)), 1e3 * float(np.mean(t_acq))
    loop_ms = B * (prep_ms + acq_ms)
    loop_ms_noprep = B * acq_ms
    out = {
        "workload": "grouped_acquisition_b%d_n%d_d32_24c8u_c%d" % (B, n, C),
        "device": torch.cuda.get_device_name(0),
        "reps": a.reps,
        "n_good": ng, "n_bad": nb,
        "acquire_ms": ms_acq, "sample_acquire_ms": ms_sa, "refit_sample_acquire_ms": ms_chain, "refit_ms": ms_fit,
        "pairs": pairs, "pairs_per_s": rate,
        "fp32_valu": {"flops_per_pair": W, "achieved_tflops": W * rate / 1e12, "peak_tflops": PEAK_FP32_TFLOPS,
                      "frac": W * rate / 1e12 / PEAK_FP32_TFLOPS},
        "mean_shortlist": float(picks.shortlist.mean()), "max_shortlist": int(picks.shortlist.max()),
        "picked": int((picks.index >= 0).sum()), "overflow_groups": int(((picks.flags & 1) != 0).sum()),
        "near_tie_groups": int(((picks.flags & 2) != 0).sum()),
        "baseline": {"subsample": int(sub.size), "prepare_ms_per_group": prep_ms, "acquire_ms_per_group": acq_ms,
                     "loop_ms_extrapolated": loop_ms, "loop_ms_extrapolated_without_prepare": loop_ms_noprep,
                     "picks_agree": agree},
        "speedup_vs_loop": loop_ms / ms_acq, "speedup_vs_loop_without_prepare": loop_ms_noprep / ms_acq,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0 if agree == sub.size and ms_acq < loop_ms else 1


if __name__ == "__main__":
    sys.exit(main())
