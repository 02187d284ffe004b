"""Single-pool acquisition by log ratio, measured (profiles/acquire_lr/README.md):

    python tools/bench_acquire_lr.py [--reps 20] [--nc 1000000] [--nobs 10000] [--out FILE.json] [--topk K]

1. config #3 (nc x nobs x 24c + 8u): KDEPair.acquire(score="log_ratio") with the fast scoring instance without the
   coarse one (the default) and with the coarse one (HBX_LR_COARSE=1), the floored acquire for context, and the only
   other route to the same pick: hbx_kde_logpdf_rtol for both KDEs plus a device argmin of ln g - ln l.
2. the generator's own call: 64 candidates against 400 and nobs observations, the bound form (acquire_pick), by log
   ratio (with and without the re-score's scan form, HBX_LR_SCAN) against the floored call.
3. a converged model (bandwidths about 1e-3) with a far pool: the log-space evaluations and the call's time over them.
--topk K: instead of the three sections, config #3's k best (profiles/topk_lr/README.md): acquire_topk(score="log_ratio"),
the only other route to that ranking -- hbx_kde_logpdf_rtol for both KDEs plus torch.topk of ln l - ln g -- and the
floored acquire_topk for context.
The routes take turns within one session; device events around every call, warmed shapes; min / median / max."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, routes, reps):
    """routes: name -> (env, fn); every route once per round, reps rounds after one warm round"""
    ms = {k: [] for k in routes}
    out = {}
    for r in range(reps + 1):
        for name, (env, fn) in routes.items():
            os.environ.update(env)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[name] = fn()
            b.record()
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    return {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ms.items()}, out


def lr_counters(pair, ws, nc):
    """(log-space evaluations, forced candidates re-scored) of the last log-ratio call on ws"""
    end = pair.workspace_bytes(nc, "log_ratio")
    return [int(v) for v in ws[end - 256:end - 248].view(__import__("torch").int32).cpu().numpy()]


def fit(kde, S, n, dev, cluster=False):
    X = S.make_observations(n, 24, 8, 4)
    if cluster:
        X[:, :24] = 0.5 + 1e-3 * np.random.RandomState(1).randn(n, 24)
    return X, kde.fit_pair(X, S.make_losses(n), S.var_type_string(24, 8), 33, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nc", type=int, default=1000000)
    ap.add_argument("--nobs", type=int, default=10000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--topk", type=int, default=0)
    a = ap.parse_args()
    import torch
    from hpbandster_amd import _native as N
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    dev = torch.device("cuda", 0)
    L = N.lib()
    res = {"nc": a.nc, "nobs": a.nobs, "reps": a.reps}
    LRD, LRC = {"HBX_LR_COARSE": "0", "HBX_LR_SCAN": "1"}, {"HBX_LR_COARSE": "1", "HBX_LR_SCAN": "1"}

    # 1. config #3
    _, pair = fit(kde, S, a.nobs, dev)
    cands = torch.from_numpy(S.make_candidates(a.nc, 24, 8, 4)).to(dev)
    ws = torch.empty(pair.workspace_bytes(a.nc, "log_ratio"), dtype=torch.uint8, device=dev)
    lg = [torch.empty(a.nc, dtype=torch.float64, device=dev) for _ in range(2)]
    sb = int(L.hbx_kde_logpdf_rtol_scratch_bytes(a.nc))
    scr = torch.empty(sb, dtype=torch.uint8, device=dev)
    sh = N.stream_handle(None, dev)

    def lnpdf_argmin():
        for k, o in zip((pair.good, pair.bad), lg):
            N.check(L.hbx_kde_logpdf_rtol(N.ptr(cands), a.nc, 32, N.ptr(k.params), N.ptr(k.table), N.ptr(k.X_dev),
                                          N.ptr(k.rows_dev), k.dc_pad, k.du_pad, k.variant, 1e-5, N.ptr(o), N.ptr(scr),
                                          sb, sh))
        s = lg[1] - lg[0]
        return int(torch.argmin(torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s)).item())

    if a.topk:
        K = a.topk
        wk = torch.empty(pair.topk_workspace_bytes(a.nc, K, "log_ratio"), dtype=torch.uint8, device=dev)

        def lnpdf_topk():
            lnpdf_argmin()
            d = lg[0] - lg[1]  # the K largest ln l - ln g are the K smallest s; NaN never
            return torch.topk(torch.where(torch.isnan(d), torch.full_like(d, -float("inf")), d), K).indices.cpu().numpy()

        routes = {"topk_log_ratio": ({}, lambda: pair.acquire_topk(cands, K, workspace=wk, score="log_ratio")),
                  "lnpdf_topk": ({}, lnpdf_topk),
                  "topk_floored": ({}, lambda: pair.acquire_topk(cands, K, workspace=wk))}
        t, out = timed(torch, routes, a.reps)
        top = pair.acquire_topk(cands, K, workspace=wk, score="log_ratio")
        ls, forced = lr_counters(pair, wk, a.nc)
        other = out["lnpdf_topk"]
        t["topk_log_ratio"].update(shortlist=top.shortlist, flags=top.flags, logspace=ls, forced=forced,
                                   first=[int(i) for i in top.index[:4]], rel_max=float(np.max(top.rel)),
                                   same_set_as_lnpdf_topk=bool(set(top.index.tolist()) == set(other.tolist())))
        t["topk_floored"].update(shortlist=out["topk_floored"].shortlist, first=[int(i) for i in out["topk_floored"].index[:4]])
        res["config3_topk_%d" % K] = t
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    routes = {"log_ratio": (LRD, lambda: pair.acquire(cands, workspace=ws, score="log_ratio")),
              "log_ratio_coarse": (LRC, lambda: pair.acquire(cands, workspace=ws, score="log_ratio")),
              "floored": ({}, lambda: pair.acquire(cands, workspace=ws)),
              "lnpdf_argmin": ({}, lnpdf_argmin)}
    t, out = timed(torch, routes, a.reps)
    for name, env in (("log_ratio", LRD), ("log_ratio_coarse", LRC)):
        os.environ.update(env)
        r = pair.acquire(cands, workspace=ws, score="log_ratio")
        ls, forced = lr_counters(pair, ws, a.nc)
        t[name].update(index=r.index, score=r.score, shortlist=r.shortlist, near=r.near, rel=r.rel, logspace=ls,
                       forced=forced, forced_share=forced / float(a.nc))
    t["floored"].update(index=out["floored"].index, score=out["floored"].score, shortlist=out["floored"].shortlist)
    t["lnpdf_argmin"].update(index=out["lnpdf_argmin"])
    res["config3"] = t
    print(json.dumps({"config3": t}), flush=True)
    del cands, ws, lg, scr

    # 2. the generator's call: 64 candidates, the bound form
    res["get_config"] = {}
    for n in (400, a.nobs):
        _, p = fit(kde, S, n, dev)
        c64 = p.good.sample(np.array([0] * 24 + [4] * 8), 3, 64, 5, 0)[0]
        w64 = torch.empty(p.workspace_bytes(64, "log_ratio"), dtype=torch.uint8, device=dev)
        row = np.empty(32)
        routes = {"floored": ({}, lambda: p.acquire_pick(c64, None, w64, row)),
                  "log_ratio_scan": (LRD, lambda: p.acquire_pick(c64, None, w64, row, score="log_ratio")),
                  "log_ratio_list": ({"HBX_LR_COARSE": "0", "HBX_LR_SCAN": "0"},
                                     lambda: p.acquire_pick(c64, None, w64, row, score="log_ratio"))}
        t, out = timed(torch, routes, 10 * a.reps)
        for k in t:
            t[k].update(index=out[k].index, shortlist=out[k].shortlist)
        res["get_config"][str(n)] = t
        print(json.dumps({"get_config_%d" % n: t}), flush=True)
    os.environ.update(LRD)

    # 3. a converged model: the log-space kernel
    Xc, pc = fit(kde, S, a.nobs, dev, cluster=True)
    rs = np.random.RandomState(2)
    far = np.concatenate((0.5 + rs.uniform(0.15, 0.4, size=(64, 1)) * np.sign(rs.randn(64, 24)),
                          rs.randint(0, 4, size=(64, 8))), axis=1).astype(np.float64)
    cf = torch.from_numpy(far).to(dev)
    wf = torch.empty(pc.workspace_bytes(64, "log_ratio"), dtype=torch.uint8, device=dev)
    t, out = timed(torch, {"log_ratio": (LRD, lambda: pc.acquire(cf, workspace=wf, score="log_ratio"))}, a.reps)
    ls, forced = lr_counters(pc, wf, 64)
    r = out["log_ratio"]
    t["log_ratio"].update(index=r.index, score=r.score, shortlist=r.shortlist, logspace=ls, forced=forced,
                          bw_max=float(np.max(pc.good.bw[:24])), ms_per_eval_upper=t["log_ratio"]["median"] / max(ls, 1))
    res["converged"] = t
    print(json.dumps({"converged": t}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
