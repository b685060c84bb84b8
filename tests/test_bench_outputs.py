"""bench.py --dump-outputs and the plain / --full split.

dump_outputs writes the timed path's output buffer as a float32 / float64 .npy: whole when it
fits the budget, else at positions fixed by the length alone (both edges and seeded draws), so
two builds write comparable files.  On the device a plain run of the plumbing case (cfg1, the
bit-exact kernel, 2^20 samples: the whole output fits) must dump exactly what the restatement
computes for the last timed step and must not run any of the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import torch
    x = np.arange(1000, dtype=np.float32)
    info = bench.dump_outputs(str(tmp_path / "d" / "out.npy"), torch.from_numpy(x), torch)
    got = np.load(tmp_path / "d" / "out.npy")
    assert got.dtype == np.float32 and got.tobytes() == x.tobytes()
    assert info["shape"] == [1000] and info["of_elements"] == 1000

    # complex128 above the budget: (re, im) rows in float64, both edges whole, sorted seeded draws between
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 16 * 3 * bench.DUMP_EDGE)
    n = 8 * bench.DUMP_EDGE
    z = (np.arange(n) + 1j * (np.arange(n) + 0.5)).astype(np.complex128)
    paths = [str(tmp_path / f"z{k}.npy") for k in range(2)]
    for p in paths:
        bench.dump_outputs(p, torch.from_numpy(z), torch, world=2)
    a, b = np.load(paths[0]), np.load(paths[1])
    assert a.dtype == np.float64 and a.shape == (3 * bench.DUMP_EDGE, 2)
    assert a.nbytes * 2 <= bench.DUMP_MAX_BYTES
    assert a.tobytes() == b.tobytes()
    idx = a[:, 0].astype(np.int64)  # the real part is the element's position
    assert np.array_equal(a[:, 1], idx + 0.5)
    assert np.array_equal(idx[: bench.DUMP_EDGE], np.arange(bench.DUMP_EDGE))
    assert np.array_equal(idx[-bench.DUMP_EDGE:], np.arange(n - bench.DUMP_EDGE, n))
    mid = idx[bench.DUMP_EDGE: -bench.DUMP_EDGE]
    assert np.all(np.diff(mid) >= 0) and mid[0] >= bench.DUMP_EDGE and mid[-1] < n - bench.DUMP_EDGE


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import oracle_lib as O
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "1", "--steps", "3",
                        "--warmup", "1", "--settle-ms", "0", "--dump-outputs", str(tmp_path)],
                       cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["full"] is False
    assert line["unit"] == "Msamples/sec" and line["higher_is_better"] is True
    # value = samples per step / ms_per_step, both as printed: ms_per_step to 1e-4 ms, value to 0.1
    rate = lambda ms: (1 << 20) / (ms * 1e-3) / 1e6
    ms = line["ms_per_step"]
    assert rate(ms + 5.1e-5) - 0.051 <= line["value"] <= rate(ms - 5.1e-5) + 0.051
    # none of the --full legs ran
    assert "cpu_baseline" not in line and "dropin" not in line and line["gather"] is None
    assert line["parity"]["value"] is None and line["parity"]["ok"] is None
    assert line["roofline"]["stream_copy_GBps"] is None
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float32 and got.shape == (1 << 20,)
    # every step filters the same 2^20 inputs on the same handle: from the second step on the
    # delay line holds the block's own tail, so the last step's output is the restatement's second block
    h = O.firdes_kaiser(63, 0.2, 60.0, 0.0).astype(np.float32)
    x = O.synth(bench.SEED, 0, 0, 1 << 20)
    f = O.fir(O.RR32, h, np.float32(1.0))
    f.execute_block(x)
    ref = f.execute_block(x)
    assert got.tobytes() == ref.tobytes()
