"""Digests of everything the grouped calls write, for a byte comparison of two libhbx builds (GPU box):

    python tools/lib_ab.py 1 tree,ab/libhbx_<name>.so tools/groups_bytes.py

For fixed seeds and the shapes (dc, du, levels) of SHAPES -- four ragged groups each -- it runs acquire,
acquire_requests under either screen, acquire_topk and logpdf in both modes into zero-filled workspaces of its own and
prints one JSON line of SHA-256 digests: the result bytes; the workspace from byte 256 on (the GScreen slots and, for
top-k, the pdf spill); ln_l, ln_g, status and the four counters (the line also carries the counters and the status
words themselves, to show which passes ran).  The ln-pdf's list region is not hashed: its order depends on atomics.
With 4 levels the categorical bandwidths exceed 1 -- at (5, 2) in the smallest group, at (24, 8) in every group: signed
sums in the screens, the exact pdf in the ln-pdf; with 2 or 3 levels they stay below 1, so (12, 3, 2), (24, 8, 2) and
(40, 6, 3) take the ln-pdf's fp32 and fp64 passes through the 16-slot, the 32-slot and the 64 + 32-slot instances.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hpbandster_amd import _native as N  # noqa: E402
from hpbandster_amd import groups  # noqa: E402
from hpbandster_amd import synthetic as S  # noqa: E402

SHAPES = [(5, 2, 4), (12, 3, 2), (24, 8, 4), (24, 8, 2), (40, 6, 3)]
REQ, C, K = 3, 70, 16


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def one_shape(dev, dc, du, lev, out):
    D = dc + du
    lens = np.array([D + 2, 70, 200, 330])
    B = len(lens)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = S.make_observations(int(seg[-1]), dc, du, lev, seed=51)
    gm = groups.fit_groups(X, S.make_losses(int(seg[-1]), seed=52), seg, S.var_type_string(dc, du), device=dev)
    rs = np.random.RandomState(53)
    P = REQ * C
    cands = S.make_candidates(B * P, dc, du, lev, seed=54).reshape(B, P, D)
    for b in range(B):
        k = rs.rand(P)
        src = X[seg[b]:seg[b + 1]][rs.randint(0, lens[b], size=P)]
        cands[b, k < 0.5] = src[k < 0.5]
        cands[b, k < 0.25, :dc] += 0.01 * rs.randn(int((k < 0.25).sum()), dc)
        far = (k >= 0.5) & (k < 0.6)
        cands[b, far, :dc] = 4.0 + rs.rand(int(far.sum()), dc)
    cd = torch.from_numpy(np.ascontiguousarray(cands.reshape(B, REQ, C, D))).to(dev)
    pool0 = cd[:, 0].contiguous()
    tag = "%dc%du/%d" % (dc, du, lev)

    def zeros(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    ws = zeros(gm.workspace_bytes(C))
    res = gm.acquire(pool0, workspace=ws, sync=False)
    torch.cuda.synchronize()
    out[tag + " acquire"] = [sha(res), sha(ws[256:])]
    for screen in ("1", "2"):
        os.environ["HBX_GROUPS_SCREEN"] = screen
        ws = zeros(gm.workspace_bytes(C, REQ))
        res = gm.acquire_requests(cd, workspace=ws, sync=False)
        torch.cuda.synchronize()
        out[tag + " requests screen " + screen] = [sha(res), sha(ws[256:])]
    os.environ.pop("HBX_GROUPS_SCREEN", None)
    ws = zeros(gm.workspace_bytes_topk(C, K))
    res = gm.acquire_topk(pool0, K, workspace=ws, sync=False)
    torch.cuda.synchronize()
    out[tag + " topk"] = [sha(res), sha(ws[256:])]
    for fp64_only in (False, True):
        ws = zeros(gm.workspace_bytes_logpdf(C))
        r = gm.logpdf(pool0, fp64_only=fp64_only, workspace=ws, sync=False)
        stats = np.zeros(4, dtype=np.int64)
        N.check(N.lib().hbx_kde_logpdf_groups_stats(N.ptr(ws), stats.ctypes.data))
        out[tag + (" logpdf fp64_only" if fp64_only else " logpdf")] = [
            sha(r.ln_l), sha(r.ln_g), sha(r.status), [int(v) for v in stats], r.status.cpu().numpy().tolist()]


def main():
    dev = torch.device("cuda", 0)
    out = {}
    for dc, du, lev in SHAPES:
        one_shape(dev, dc, du, lev, out)
    print(json.dumps(out, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
