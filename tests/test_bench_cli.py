"""bench.py's command line: a plain run times only its headline steps, --full
adds the legs around it, --dump-outputs writes the last step's result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gxlib import GX_TPCH_LINEITEM, load_oracle
from tidb_amd import plan as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_layout(tmp_path):
    import bench
    rows = [("A", "F", "123.4500", 7), (None, "NO", None, None)]
    bench.dump_outputs(str(tmp_path), "t", ["k0", "k1", "dec", "cnt"],
                       [4, 4, 2, 0], rows)
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["t_cnt.npy", "t_dec.npy", "t_k0.npy", "t_k1.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["t_k0.npy"], [[65.0], [np.nan]])
    np.testing.assert_array_equal(got["t_k1.npy"], [[70.0, -1.0], [78.0, 79.0]])
    np.testing.assert_array_equal(got["t_dec.npy"], [123.45, np.nan])
    np.testing.assert_array_equal(got["t_cnt.npy"], [7.0, np.nan])


def test_full_option_is_off_by_default():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                          "--help"], capture_output=True, text=True, check=True)
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_q1_result(tmp_path):
    n = 200_000
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--rows", str(n),
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, check=True)
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "tpch_q1_rows_per_sec"
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] / 1000.0))
    # the legs behind --full did not run
    assert line["cpu_baseline"] is None and line["q3_sf100"] is None

    # the dump is the Q1 result: same table through the CPU oracle
    lib = load_oracle()
    b, src, agg, out_types, out_fracs = P.q1_plan(lib)
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
    ex.open()
    caps = [2048 if t == 4 else None for t in out_types]
    want = sorted(ex.pull_all(out_types, out_fracs, data_caps=caps))
    ex.close()
    ex.free()
    b.free()
    import bench
    assert sorted(os.listdir(tmp_path)) == sorted(
        f"q1_{name}.npy" for name in bench.Q1_OUT_NAMES)
    for c, name in enumerate(bench.Q1_OUT_NAMES):
        got = np.load(tmp_path / f"q1_{name}.npy")
        assert got.dtype == np.float64 and got.shape[0] == len(want)
        if c < 2:
            exp = [[float(ord(r[c]))] for r in want]
        else:
            exp = [float(r[c]) for r in want]
        np.testing.assert_array_equal(got, exp)
