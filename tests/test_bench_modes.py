"""bench.py's run modes: a plain run measures the headline figure only, --full adds the side lines, and
--dump-outputs writes the last timed step's winner record as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SMALL = ["--candidates", "5000", "--obs", "400", "--dc", "6", "--du", "2", "--levels", "3"]


def test_plain_is_the_default():
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "d"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (True, "d", 7, 2)


def test_dump_outputs_files(tmp_path):
    class Rec(object):
        index, score, pdf_l, pdf_g = 2 ** 40 + 3, 0.1, 1.5e-7, float("inf")

    d = str(tmp_path / "a" / "b")  # created on demand
    bench.dump_outputs(d, Rec, 1)
    assert sorted(os.listdir(d)) == ["index.npy", "pdf_g.npy", "pdf_l.npy", "score.npy"]
    for name in ("index", "score", "pdf_l", "pdf_g"):
        v = np.load(os.path.join(d, name + ".npy"))
        assert v.dtype == np.float64 and v.shape == (1,)
        assert v[0] == getattr(Rec, name)
    d2 = str(tmp_path / "c")
    bench.dump_outputs(d2, Rec, 2)  # several ranks: the exchanged (score, index) only
    assert sorted(os.listdir(d2)) == ["index.npy", "score.npy"]


@pytest.mark.gpu
def test_plain_run_line_and_dump(device, tmp_path):
    """A plain run at a small shape: the line's headline fields, no side line, --steps timed steps, and the
    dumped record bit for bit what pair.acquire returns for the same seeded inputs."""
    import torch
    from hpbandster_amd import kde
    from hpbandster_amd import synthetic as S
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", d] + SMALL, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["roofline"]["launch_ms_stats"]["samples"] == 3
    assert line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    for k in ("config5", "config2", "config4_single_gpu", "precise_logpdf", "refit", "promote_dropin"):
        assert k not in line, k
    X = S.make_observations(400, 6, 2, 3)
    pair = kde.fit_pair(X, S.make_losses(400), S.var_type_string(6, 2), 9, device=device)
    res = pair.acquire(torch.from_numpy(S.make_candidates_blocked(0, 5000, 6, 2, 3)).to(device))
    assert line["config"]["winner"] == res.index
    for name in ("index", "score", "pdf_l", "pdf_g"):
        v = np.load(os.path.join(d, name + ".npy"))
        assert v.dtype == np.float64 and v.shape == (1,)
        assert v[0] == getattr(res, name), name
