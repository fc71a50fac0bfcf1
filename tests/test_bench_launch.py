"""bench.py's launcher contract on CPU: ``--gpus N`` without a launcher starts N ranks through
torch.distributed.run (the parent never touches the GPU), and a launcher world size that differs from
--gpus is refused before any GPU call."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, env=None, timeout=180):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=e, timeout=timeout, cwd=ROOT)


def test_self_launch_starts_n_ranks():
    r = _run(["--gpus", "2", "--launch-probe"])
    assert r.returncode == 0, r.stderr[-2000:]
    seen = sorted(json.loads(l)["rank"] for l in r.stdout.splitlines() if l.startswith("{"))
    worlds = {json.loads(l)["world"] for l in r.stdout.splitlines() if l.startswith("{")}
    assert seen == [0, 1] and worlds == {2}, r.stdout


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--launch-probe"], env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr


def test_single_rank_default():
    r = _run(["--launch-probe"])
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1]) == {"rank": 0, "world": 1}


def test_full_and_dump_outputs_are_options():
    r = _run(["--help"])
    assert r.returncode == 0 and "--full " in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """A plain run times the headline step and nothing else: one result line without the --full sub-records, and
    --dump-outputs writes the last step's SC message bits (a fixed sample) and both decoders' counters, whose SC
    counts equal the errors of the dumped bits' step times the number of timed steps."""
    import numpy as np
    steps, B = 3, 8192
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B), "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["steps"] == steps and d["higher_is_better"] is True and d["unit"].startswith("codewords/s")
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 5 * B) < 1e-3 * 5 * B
    assert "configs_summary" not in d and "cpu_baseline" not in d and "full_record" not in d
    out = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(out) == ["gru_counts", "sc_counts", "sc_msg_hat", "sc_msg_hat_rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["sc_msg_hat"].shape == (5, B, 32) and set(np.unique(out["sc_msg_hat"])) == {-1.0, 1.0}
    assert np.array_equal(out["sc_msg_hat_rows"], np.arange(B))
    assert out["sc_counts"].shape == out["gru_counts"].shape == (5, 2)
    assert np.all(out["sc_counts"] % steps == 0) and np.all(out["gru_counts"] % steps == 0)
    assert np.all(out["sc_counts"][:, 1] / steps <= B) and out["sc_counts"][0, 1] > out["sc_counts"][4, 1] > 0
    assert d["sc_bler"]["0.0"] == pytest.approx(out["sc_counts"][0, 1] / (steps * B), rel=1e-4)


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_rehearsal(tmp_path):
    """The N > 1 bench path end to end on one MI355X (the driver's 8-GPU scaling run uses it over RCCL): two ranks
    launched by bench.py itself, both on cuda:0 over gloo (NPD_BENCH_SHARE_GPU / NPD_BENCH_BACKEND), weak scaling --
    rank 0 prints one line whose value counts both ranks' codewords, with per-rank times and a 2-rank world."""
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "65536", "--full", "--no-traffic",
              "--no-cpu-baseline", "--no-gru", "--no-pac", "--no-conv", "--no-scl", "--no-lse", "--no-mc",
              "--full-json", str(tmp_path / "bench_full_2rank.json")],
             env={"NPD_BENCH_BACKEND": "gloo", "NPD_BENCH_SHARE_GPU": "1"}, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["n_gpus"] == 2 and d["world_size_rccl"] == 2 and len(d["rank_ms_per_step"]) == 2
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 2 * 5 * 65536) < 1e-3 * 2 * 5 * 65536
    assert d["configs_summary"]["1_sc_decode"]["ber_match_0.05dB"] is not None
