"""bench.py as it is run for every change: a plain run (set-up, warm-up, the timed steps, one JSON line) in a fresh process,
its --dump-outputs records against a blocking run of the same seeded batch in this process, and the line's headline fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--min-seconds", "0.3",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["metric"] == "SV loci validated/sec" and d["unit"] == "loci/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] > 0 and d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] == pytest.approx(d["timed_region_s"] * 1e3 / 3, rel=1e-3)
    for k in ("roofline", "cpu_baseline", "inclusive", "sub", "files_path", "pipeline", "hits_per_pass", "kernel_source_id"):
        assert k not in d, k                                        # (behind --full)

    rec = np.load(out / "loci_records.npy")
    from vapor_amd import workload as wl
    from vapor_amd.engine import Engine
    spec = wl.WORKLOADS["cfg2"]
    w = wl.make_workload("cfg2", seed=1000, **spec)                 # (bench.py's batch on rank 0)
    assert rec.dtype == np.float64 and rec.shape == (w.n_loci, 8)
    eng = Engine(0)
    try:
        ss = w.upload(eng)
        p = eng.plan(ss, w.pairs)
        p.set_reads(wl.read_table(w), w.n_loci)
        exp = p.run_loci().copy()
        p.close()
        ss.close()
    finally:
        eng.close()
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(rec), nan)
    assert np.allclose(rec[~nan], exp[~nan], rtol=0, atol=1e-9)
    assert d["loci_with_scores"] == int((~nan[:, 0]).sum()) > 0
