"""The top-k acquisition of one pool, unstaged against staged (HBX_STAGED=0 / 2 / unset), alternating in one
process: wall time per call, each call ending with its result block on the host, the call's stage counts and the
header's `shortlist`, one JSON line per (shape, k) (profiles/staged_topk/README.md).

    python tools/bench_topk.py [--shapes config3,config2,config2u,noprune] [--ks 1,8,64,1024] [--parent-lib PATH]
    python tools/bench_topk.py --shapes threshold --ks 64     # unsigned 24c + 8u pairs, Nc = 100 x observations

--parent-lib: another build of libhbx.so (the parent commit's) whose hbx_kde_acquire_topk is called on the same
prepared pair, candidates and workspace, alternated with this tree's.  The staged and unstaged blocks -- and the
other library's -- are checked equal field by field (count, flags, index, score, pdf_l, pdf_g, rel); a mismatch
ends the run with exit status 1.  Every timed call, this tree's included, is the same native call from this file
(topk_with), so the libraries differ in nothing but their code.  For config #3 the staged single `acquire`, the
floor of the staged top-k, is timed as well.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hpbandster_amd import _native as N  # noqa: E402
from hpbandster_amd import kde  # noqa: E402
from hpbandster_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)
WARM, REPS = 5, 20
FIELDS = ("index", "score", "pdf_l", "pdf_g", "rel")

# name: (dc, du, levels, observations, candidates, blocked candidate stream, categorical bandwidths capped)
SHAPES = {
    "config3": (24, 8, 4, 10000, 1000000, True, False),
    "config2": (24, 8, 4, 1000, 100000, False, False),  # as fitted: a signed good KDE, which does not stage
    "config2u": (24, 8, 4, 1000, 100000, False, True),  # config #2's size with both KDEs unsigned: it stages
    "noprune": (8, 0, 1, 10000, 1000000, False, False),  # pdfs far above 1e-8: every l-only bound below any score
}
# the threshold sweep (tools/staged_onoff.py threshold): unsigned pairs, Nc = 100 x observations, 1e8 .. 4.9e9 pairs
for _n in (1000, 2000, 3000, 4000, 5000, 7000):
    SHAPES["thr%d" % _n] = (24, 8, 4, _n, 100 * _n, False, True)


def set_mode(mode):
    if mode == "unset":
        os.environ.pop("HBX_STAGED", None)
    else:
        os.environ["HBX_STAGED"] = mode


def other_lib(path):
    L = ctypes.CDLL(path)
    res, args = N.SIGNATURES["hbx_kde_acquire_topk"]
    L.hbx_kde_acquire_topk.restype, L.hbx_kde_acquire_topk.argtypes = res, args
    return L


def unsigned_pair(X, losses, dc, du):
    """BOHB's split with normal-reference bandwidths, the categorical ones capped at 0.8: both KDEs unsigned."""
    from oracle import kde_oracle as O
    vt = S.var_type_string(dc, du)
    g_idx, b_idx = O.bohb_split(X, losses, dc + du + 1)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    bwg[dc:] = np.minimum(bwg[dc:], 0.8)
    bwb[dc:] = np.minimum(bwb[dc:], 0.8)
    return kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt), device=dev)


def topk_with(L, pair, C, k, ws, out):
    """pair.acquire_topk's native call through library L, the block fetched to the host."""
    rc = L.hbx_kde_acquire_topk(C.data_ptr(), C.shape[0], k, 0, pair._bound, out.data_ptr(), ws.data_ptr(),
                                ws.numel(), N.stream_handle(None, dev))
    if rc != 0:
        raise RuntimeError("hbx_kde_acquire_topk: error %d" % rc)
    return kde.TopK.from_bytes(kde.fetch_bytes(out, None))


def timed(fn):
    """(median, min, max) wall ms of REPS calls behind WARM warm-up calls, and the last result."""
    for _ in range(WARM):
        r = fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)], r


def same(a, b):
    return (a.count, a.flags) == (b.count, b.flags) and \
        all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIELDS)


def run_shape(name, ks, parent, rounds):
    dc, du, levels, nobs, nc, blocked, capped = SHAPES[name]
    X = S.make_observations(nobs, dc, du, levels)
    if capped:
        pair = unsigned_pair(X, S.make_losses(nobs), dc, du)
    else:
        pair = kde.fit_pair(X, S.make_losses(nobs), S.var_type_string(dc, du), dc + du + 1, device=dev)
    tree = N.lib()
    Ch = S.make_candidates_blocked(0, nc, dc, du, levels) if blocked else S.make_candidates(nc, dc, du, levels)
    C = torch.from_numpy(Ch).to(dev)
    ok = True
    for k in ks:
        ws = torch.empty(pair.topk_workspace_bytes(nc, k), dtype=torch.uint8, device=dev)
        out = torch.empty(int(N.lib().hbx_kde_topk_result_bytes(k)), dtype=torch.uint8, device=dev)
        rec = {"shape": name, "dc": dc, "du": du, "obs": nobs, "cand": nc, "k": k,
               "variants": [int(pair.good.variant), int(pair.bad.variant)]}
        blocks = {}
        for rnd in range(rounds):
            for mode in ("0", "2", "unset"):
                set_mode(mode)
                ms, top = timed(lambda: topk_with(tree, pair, C, k, ws, out))
                rec["mode%s_r%d" % (mode, rnd)] = {"ms": ms, "stats": pair.acquire_stats(ws, nc),
                                                   "shortlist": top.shortlist, "flags": top.flags}
                blocks["mode" + mode] = top
            if parent is not None:
                set_mode("unset")
                ms, top = timed(lambda: topk_with(parent, pair, C, k, ws, out))
                rec["parent_r%d" % rnd] = {"ms": ms, "shortlist": top.shortlist, "flags": top.flags}
                blocks["parent"] = top
        rec["equal"] = {n: same(blocks["mode0"], b) for n, b in blocks.items() if n != "mode0"}
        ok = ok and all(rec["equal"].values())
        print(json.dumps(rec), flush=True)
    if name == "config3":  # the floor: the staged single acquisition on the same pair and candidates
        ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=dev)
        rec = {"shape": name, "call": "acquire"}
        for rnd in range(rounds):
            for mode in ("0", "unset"):
                set_mode(mode)
                ms, r = timed(lambda: pair.acquire(C, workspace=ws))
                rec["mode%s_r%d" % (mode, rnd)] = {"ms": ms, "stats": pair.acquire_stats(ws, nc),
                                                   "shortlist": r.shortlist, "index": r.index}
        print(json.dumps(rec), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="config3,config2,config2u,noprune")
    ap.add_argument("--ks", default="1,8,64,1024")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args(argv)
    shapes = a.shapes.split(",")
    if shapes == ["threshold"]:
        shapes = sorted((s for s in SHAPES if s.startswith("thr")), key=lambda s: int(s[3:]))
    for s in shapes:
        if s not in SHAPES:
            ap.error("unknown shape %r (of %s)" % (s, ", ".join(sorted(SHAPES))))
    ks = [int(k) for k in a.ks.split(",")]
    if any(k < 1 or k > kde.TOPK_MAX_K for k in ks):
        ap.error("k outside [1, %d]" % kde.TOPK_MAX_K)
    parent = other_lib(a.parent_lib) if a.parent_lib else None
    ok = True
    for s in shapes:
        ok = run_shape(s, ks, parent, a.rounds) and ok
    set_mode("unset")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
