"""bench.py --dump-outputs and --full on the GPU: the dump is the IQ the timed transmit path left on
the device (a seeded sample of the batch's subframes once it exceeds the size budget), identical
to what TxPipeline gives a caller for the bench's inputs; a plain run makes none of the side runs
and --full makes them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_SF = 128           # C3: 128 subframes x 2 antennas x 30720 samples exceed the budget, so rows are sampled


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--settle-ms", "0", "--batch", str(N_SF), *args], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_timed_paths_iq(gpu, tmp_path):
    import bench
    from openair4g_amd import dist as odist
    out = _bench("--dump-outputs", str(tmp_path / "d"))
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["roofline"] is None and out["cpu_baseline"] is None      # no side runs without --full
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == ["iq.npy", "iq_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in files) <= 64 << 20
    iq, rows = np.load(tmp_path / "d" / "iq.npy"), np.load(tmp_path / "d" / "iq_rows.npy")
    assert iq.dtype == np.float32 and rows.dtype == np.float64
    rows = rows.astype(np.int64)
    assert 1 < len(rows) < N_SF and len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < N_SF
    assert bench.DUMP_BUDGET <= 64 << 20 and iq.nbytes <= bench.DUMP_BUDGET
    # the same inputs through the library in this process: the arrays a caller receives
    p = gpu.make_params("C3", subframe=7)
    pipe = gpu.TxPipeline(p, N_SF)
    pipe.fill_payload(seed=odist.global_payload_seed(0x5EED0000, 0, p))
    pipe.run()
    pipe.sync()
    want = pipe.iq()[rows].reshape(len(rows), -1).view(np.int16)
    pipe.close()
    assert iq.shape == want.shape
    assert np.array_equal(iq, want.astype(np.float32))
    assert np.count_nonzero(iq) > iq.size // 2


def test_full_run_adds_the_side_runs(gpu):
    # the CPU baseline leg itself (seconds of host work) is covered by tests/test_bench_cpu.py
    out = _bench("--full", "--no-cpu-baseline", "--kernel-reps", "2", "--config", "C1")
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert set(out["roofline"]["kernel_ms"]) == {"encode_rm_scramble", "modulate_idft_cp"}
    assert all(v > 0 for v in out["roofline"]["kernel_ms"].values()) and out["roofline"]["frac"] > 0
    assert out["cpu_baseline"] is None
