"""bench.py's command line: a plain run does the headline only and can dump
what its last timed step returned; everything else sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ret", "pbs_stat", "dbs_stat", "obj_val", "it_cnt", "some", "row_stat", "col_stat", "row_prim", "col_prim",
         "row_dual", "col_dual")


def test_dump_outputs_writes_float64_arrays(tmp_path):
    """dump_outputs: one float64 .npy per name of GkProblem.result() plus the
    return code; other ranks under their own suffix."""
    sys.path.insert(0, ROOT)
    import bench
    res = dict(pbs_stat=2, dbs_stat=2, obj_val=1.5, it_cnt=7, some=0,
               row_stat=np.array([1, 2], np.int8), col_stat=np.array([2, 1, 1], np.int8),
               row_prim=np.array([0.5, 0.25]), col_prim=np.zeros(3), row_dual=np.zeros(2),
               col_dual=np.array([1.0, -2.0, 3.0]))
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), 0, 8, res)
    bench.dump_outputs(str(out), 1, 0, res)
    assert sorted(os.listdir(out)) == sorted([n + ".npy" for n in NAMES] + [n + ".rank1.npy" for n in NAMES])
    for n in NAMES:
        a = np.load(out / (n + ".npy"))
        assert a.dtype == np.float64 and a.ndim == 1
        want = 8 if n == "ret" else res[n]
        assert np.array_equal(a, np.atleast_1d(np.asarray(want, np.float64)))
    assert np.load(out / "ret.rank1.npy")[0] == 0.0


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps(tmp_path):
    """A plain run on a small instance: --steps sets the timed steps, the
    line carries ms_per_step and none of the --full legs, and the dump holds
    the last step's arrays (2 steps after 1 warm-up of 20 pivots: it_cnt 60)."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--m", "64", "--n", "256", "--pivots-per-step", "20", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "pivots/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["extra"] == {}
    assert d["engine"]["kernels"] == {}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in NAMES)
    assert np.load(out / "row_prim.npy").shape == (64,) and np.load(out / "col_dual.npy").shape == (256,)
    # 40 timed pivots in the rate, 60 on the problem, unless the optimum came first
    ret, it = np.load(out / "ret.npy")[0], np.load(out / "it_cnt.npy")[0]
    assert ret in (0.0, 8.0)
    if ret == 8.0 and d["engine"]["restarts"] == 0:
        assert it == 60.0
        assert abs(d["value"] - 40 / (2 * d["ms_per_step"] / 1000.0)) <= 0.01 * d["value"]
