"""The staged single acquisition forced off / on (HBX_STAGED=0 / 2 / unset): stream time per call and the call's
stage counts, one JSON line per case (profiles/staged/README.md).

    python tools/staged_onoff.py sizes       # no-prune case, config #2, mid sizes, the bench shape (fit_pair)
    python tools/staged_onoff.py threshold   # unsigned 24c + 8u pairs, Nc = 100 x observations, 1e8 .. 4.9e9 pairs
    python tools/staged_onoff.py stream      # the bench's own pair and candidate stream: stage counts
    python tools/staged_onoff.py pair1       # stage 1's one-tile kernel choice: HBX_PAIR1=1 / 0 under HBX_STAGED=2
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hpbandster_amd import kde  # noqa: E402
from hpbandster_amd import synthetic as S  # noqa: E402
from oracle import kde_oracle as O  # noqa: E402

dev = torch.device("cuda", 0)


def set_mode(mode):
    if mode == "unset":
        os.environ.pop("HBX_STAGED", None)
    else:
        os.environ["HBX_STAGED"] = mode


def timed(pair, C, ws, reps, warm=5):
    """(stream ms per call, stage counts, the record's main fields) of back-to-back synchronous calls."""
    nc = C.shape[0]
    for _ in range(warm):
        r = pair.acquire(C, workspace=ws)
    st = pair.acquire_stats(ws, nc)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        r = pair.acquire(C, workspace=ws)
    b.record()
    torch.cuda.synchronize()
    return {"stream_ms_per_call": round(a.elapsed_time(b) / reps, 5), "stats": st,
            "rec": [r.index, r.score, r.shortlist, r.flags]}


def unsigned_pair(nobs, dc=24, du=8):
    """BOHB's split with normal-reference bandwidths, the categorical ones capped at 0.8: both KDEs unsigned."""
    vt = S.var_type_string(dc, du)
    X = S.make_observations(nobs, dc, du, 4)
    g_idx, b_idx = O.bohb_split(X, S.make_losses(nobs), dc + du + 1)
    bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    bwg[dc:] = np.minimum(bwg[dc:], 0.8)
    bwb[dc:] = np.minimum(bwb[dc:], 0.8)
    return kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, O.num_levels(X[g_idx], vt),
                                  O.num_levels(X[b_idx], vt), device=dev)


def run_sizes(name, dc, du, nobs, nc, reps=20):
    levels = 4 if du else 1
    X = S.make_observations(nobs, dc, du, levels)
    pair = kde.fit_pair(X, S.make_losses(nobs), S.var_type_string(dc, du), dc + du + 1, device=dev)
    C = torch.from_numpy(S.make_candidates(nc, dc, du, levels)).to(dev)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=dev)
    out = {"case": name, "dc": dc, "du": du, "obs": nobs, "cand": nc,
           "variants": [int(pair.good.variant), int(pair.bad.variant)]}
    for rnd in range(2):
        for mode in ("0", "2", "unset"):
            set_mode(mode)
            out["mode%s_r%d" % (mode, rnd)] = timed(pair, C, ws, reps, warm=3)
    print(json.dumps(out), flush=True)


def run_threshold(nobs, nc, reps=30):
    pair = unsigned_pair(nobs)
    C = torch.from_numpy(S.make_candidates(nc, 24, 8, 4)).to(dev)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=dev)
    out = {"obs": nobs, "cand": nc, "pairs": nobs * nc,
           "variants": [int(pair.good.variant), int(pair.bad.variant)]}
    for rnd in range(3):
        for mode in ("0", "2"):
            set_mode(mode)
            out["mode%s_r%d" % (mode, rnd)] = timed(pair, C, ws, reps)
    print(json.dumps(out), flush=True)


def run_stream(nobs=10000, nc=1000000, dc=24, du=8):
    """bench.py's pair (fit_pair on its observations) and candidates (rows [0, nc) of the blocked stream)."""
    X = S.make_observations(nobs, dc, du, 4)
    pair = kde.fit_pair(X, S.make_losses(nobs), S.var_type_string(dc, du), dc + du + 1, device=dev)
    C = torch.from_numpy(S.make_candidates_blocked(0, nc, dc, du, 4)).to(dev)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=dev)
    out = {"case": "bench_stream", "obs": nobs, "cand": nc}
    for mode in ("0", "unset"):
        set_mode(mode)
        out["mode%s" % mode] = timed(pair, C, ws, 20)
    print(json.dumps(out), flush=True)


def run_pair1(nobs, nc, reps=30):
    """Staged calls whose stage 1 fits one round of the chip's block slots on its own (Nc <= 262144): the
    one-tile coarse kernel (HBX_PAIR1 unset) against the two-tile one (HBX_PAIR1=0); only stage 1 differs."""
    pair = unsigned_pair(nobs)
    C = torch.from_numpy(S.make_candidates(nc, 24, 8, 4)).to(dev)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=dev)
    set_mode("2")
    out = {"case": "stage1_pair1", "obs": nobs, "cand": nc}
    for rnd in range(3):
        for p1 in ("1", "0"):
            os.environ["HBX_PAIR1"] = p1
            out["pair1_%s_r%d" % (p1, rnd)] = timed(pair, C, ws, reps)
    os.environ.pop("HBX_PAIR1", None)
    print(json.dumps(out), flush=True)


def main(argv):
    what = argv[0] if argv else "sizes"
    if what == "threshold":
        for nobs in (1000, 2000, 3000, 4000, 5000, 7000):
            run_threshold(nobs, 100 * nobs)
    elif what == "stream":
        run_stream()
    elif what == "pair1":
        for nobs, nc in ((8500, 140000), (8500, 200000), (8500, 260000)):
            run_pair1(nobs, nc)
    else:
        run_sizes("noprune_8c_1e4_1e6", 8, 0, 10000, 1000000)
        run_sizes("config2_1e5x1e3", 24, 8, 1000, 100000)
        run_sizes("mid_3e5x3e3", 24, 8, 3000, 300000)
        run_sizes("mid_4e5x4e3", 24, 8, 4000, 400000)
        run_sizes("headline", 24, 8, 10000, 1000000)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
