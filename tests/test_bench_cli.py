"""bench.py command line: a plain run is lean (no CPU-baseline leg unless
--full), --steps sets the number of timed steps, and --dump-outputs writes
what the last timed step returned, reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _u64(words):
    return [int(lo) | (int(hi) << 32) for lo, hi in words]


def test_help_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"],
                                  ["--workload", "sweep", "--dump-outputs", "x"]])
def test_bad_arguments_are_rejected(argv):
    p = subprocess.run([sys.executable, BENCH] + argv, capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2


def test_dump_q1_outputs_is_exact(tmp_path):
    import trino_amd
    r = trino_amd.Q1Result()
    for c in range(6):
        r.sum_qty[c] = c + 0.5
        r.sum_charge[c] = 1e15 + c / 3.0
        r.count[c] = 600_000_000 + c
    raw = [(0xFEDCBA9876543210 + 0x0123456789ABCDEF * i) & ((1 << 64) - 1)
           for i in range(60)]
    for i, v in enumerate(raw):
        r.raw[i] = v
    merged = list(reversed(raw))
    d = tmp_path / "out"
    bench.dump_q1_outputs(str(d), r, merged)
    names = sorted(os.listdir(d))
    assert names == sorted([f + ".npy" for f in bench.Q1_F64_FIELDS]
                           + ["count.npy", "raw.npy", "merged_raw.npy"])
    for n in names:
        assert np.load(d / n).dtype == np.float64
    assert np.load(d / "sum_qty.npy").tolist() == list(r.sum_qty)
    assert np.load(d / "sum_charge.npy").tolist() == list(r.sum_charge)
    assert np.load(d / "count.npy").tolist() == list(r.count)
    assert _u64(np.load(d / "raw.npy")) == raw
    assert _u64(np.load(d / "merged_raw.npy")) == merged


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    """One small plain run: the result line carries the headline fields, no
    CPU-baseline leg ran, and the dumped arrays are the oracle's exact Q1."""
    import oracle
    sf, steps, warmup = 0.01, 3, 1
    d = tmp_path / "dump"
    p = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps),
         "--warmup", str(warmup), "--sf-per-gpu", str(sf),
         "--dump-outputs", str(d)],
        capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "tpch_q1_scan_filter_agg_throughput"
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64"
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["ms_per_step"] > 0
    rows = out["config"]["rows_total"]
    assert out["value"] == pytest.approx(rows / (out["ms_per_step"] / 1000.0))
    assert out["cpu_baseline"] is None
    assert "cpu_baseline" not in p.stderr

    li = oracle.gen_lineitem(sf)
    assert rows == len(li["shipdate"])
    exact, _ = oracle.q1_exact(li, bench.Q1_CUTOFF)
    for f in ("sum_qty", "sum_base", "sum_disc_price", "sum_charge", "avg_disc"):
        got = np.load(d / (f + ".npy"))
        assert got.dtype == np.float64
        assert got.tolist() == list(getattr(exact, f)), f
    assert np.load(d / "count.npy").tolist() == list(exact.count)
    assert np.load(d / "raw.npy").shape == (60, 2)
    assert not (d / "merged_raw.npy").exists()
