"""bench.py's options: a plain run is lean (--full holds the CPU baseline, the den-none
passes and frame_groups), --dump-outputs writes the last timed step's arrays as float32
.npy within its budget, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_scene

import bench


def test_options_default_to_a_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_named_arrays_flattens_results():
    import torch

    from stereo_matchin_amd.pipeline import MatchResult
    t = [torch.full((2, 3), i) for i in range(9)]
    res = MatchResult(*t[:6], None, t[7], t[8])
    got = bench.named_arrays({"": res, "refine": {"final_rgba": t[0], "iters": 6}}, "pair1_")
    assert sorted(got) == ["pair1_" + n for n in ("code_ref", "code_tar", "conf_ref", "conf_tar", "cost", "d_ref",
                                                  "d_tar", "lr_red_rgba", "refine_final_rgba")]
    assert got["pair1_cost"] is t[8]
    assert sorted(bench.named_arrays({"d_ref": np.zeros(3), "timings": {"total": 1.0}})) == ["d_ref"]


def test_dump_outputs_budget_and_determinism(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000 * 4)
    monkeypatch.setattr(bench, "DUMP_MIN", 500)
    arrays = {"small": np.arange(600, dtype=np.int32).reshape(20, 30),        # whole: 500 sure + 100
              "image": (torch.arange(8000) % 256).to(torch.uint8).reshape(20, 100, 4),  # sampled
              "volume": torch.arange(100000, dtype=torch.float32).reshape(10, 100, 100)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.size for v in got.values()) <= 4000
    np.testing.assert_array_equal(got["small"], arrays["small"])
    assert got["image"].size >= 500 and got["volume"].size >= 500
    v = got["volume"]  # a sample of arange is its own sorted index list
    assert np.all(np.diff(v) >= 0) and v.min() >= 0 and v.max() < 100000 and len(np.unique(v)) > 400
    assert set(got["image"]) <= set(np.arange(256, dtype=np.float32))
    for n in arrays:
        np.testing.assert_array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(gpu, oracle, tmp_path):
    """bench.py --workload c1 (the Tsukuba pair, D16 T5 r7): the plain line has no CPU baseline and
    no den-none passes, and the dumped maps are the oracle's."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", "c1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "maps/s" and res["higher_is_better"]
    assert res["value"] == pytest.approx(1000.0 / res["ms_per_step"], rel=1e-3)
    assert res["cpu_baseline"] is None and res["roofline"]["v_none_ms"] is None and "frame_groups" not in res
    L, R, _ = load_scene("tsukuba")
    ref = oracle.match(L, R, 16, 5, 7)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"d_ref", "d_tar", "conf_ref", "conf_tar", "code_ref", "code_tar", "lr_rgba", "lr_red_rgba", "cost"} <= set(got)
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64e6
    np.testing.assert_array_equal(got["d_ref"], ref["d_ref"])
    np.testing.assert_array_equal(got["d_tar"], ref["d_tar"])
    np.testing.assert_array_equal(got["lr_red_rgba"], ref["lr_red_rgba"])
