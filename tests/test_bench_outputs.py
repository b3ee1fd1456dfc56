"""bench.py's plain run: only the timed steps, the result line, and with ``--dump-outputs``
the arrays the timed call left (last sample row, chain state), reproducible from the seeds."""

import json
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

W, K, CHAINS = 3, 4, 64


def test_extra_legs_are_opt_in(monkeypatch):
    """Without ``--full`` nothing beside the timed steps is asked for; the legs' own switches
    stay accepted so that old command lines keep working."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-pmc", "--cpu-seconds", "0",
                                      "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_pmc and a.cpu_seconds == 0 and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu_lib, tmp_path):
    """One plain run of a 64-chain cfg 3: the line carries the headline figures and none of
    the --full legs; the dumped arrays are float64 and equal, bit for bit, what the same
    seeded engine computes in this process (a launch per call: results do not depend on the
    resident launch, tests/test_gpu_resident.py)."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(K), "--warmup", str(W), "--chains", str(CHAINS),
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == K and line["warmup"] == W and line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["config"]["recorded_iters_in_timed_region"] == K
    G = bench.WORKLOADS["cfg3"]["groups"]
    # value = chains x groups x K / t and ms_per_step = t / K: the same timed region
    assert line["ms_per_step"] > 0
    assert line["ms_per_step"] * line["value"] == pytest.approx(1e3 * CHAINS * G, rel=1e-9)

    wl = dict(bench.WORKLOADS["cfg3"], chains=CHAINS, name="cfg3")
    eng, _, _ = bench.make_engine(wl, 0, 1, 0)
    eng.set_schedule(*bench.bench_schedule(W, K))
    eng.run(0, W)
    eng.run(W, W + K)
    want = {"sample_row": eng.samples_raw(K - 1, 1)[0].T}
    st = eng.get_state()
    eng.close()
    for name in ("value", "log_prior", "ll", "scale", "mu", "s2"):
        want["state_" + name] = st[name]

    got = {f[:-len(".npy")]: numpy.load(str(out / f)) for f in sorted(os.listdir(str(out)))}
    assert sorted(got) == sorted(want)
    for name, a in got.items():
        assert a.dtype == numpy.float64 and numpy.isfinite(a).all(), name
        assert a.shape == want[name].shape and numpy.array_equal(a, want[name]), name
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
