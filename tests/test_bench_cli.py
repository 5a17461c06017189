"""bench.py's command line: the plain run (set up, warm up, time, report), the
legs behind --full, and --dump-outputs.  CPU cases run the oracle-backed stub
(--cpu-stub, tests/bench_stub.py); the GPU case compares a dump with the
detector's own outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "cpu_baseline", "parity", "gpu_vs_cpu", "pcie_inclusive", "kernels", "result_gather",
             "multi_context", "exact_no_shortcuts", "host_beat_stages", "dropin_latency", "draft_undecided",
             "real_envelope_detection")
DUMP_NAMES = ("n_troughs", "n_peaks", "flags", "recording_ids", "sample", "sample_offsets", "env", "floor",
              "troughs", "peaks")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *argv],
                       capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in DUMP_NAMES)
    out = {n: np.load(os.path.join(d, n + ".npy"), allow_pickle=False) for n in DUMP_NAMES}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def test_dump_sample_is_seeded_and_within_budget():
    import bench
    sizes = [1000 + 37 * (i % 11) for i in range(500)]
    a = bench.dump_sample(sizes, budget=100_000)
    assert a == bench.dump_sample(list(sizes), budget=100_000) == sorted(set(a))
    assert 0 < len(a) < 500 and sum(sizes[i] for i in a) <= 100_000
    assert a != list(range(len(a)))                                 # a sample over the batch, not its head
    assert bench.dump_sample(sizes, budget=10 ** 9) == list(range(500))
    assert bench.dump_sample(sizes, budget=0) == []
    assert bench.DUMP_BUDGET + (1 << 20) <= 64 * 10 ** 6            # payload + .npy headers stay under 64 MB


def test_dump_outputs_layout(tmp_path, monkeypatch):
    import bench
    rng = np.random.default_rng(3)
    host = []
    for f in range(6):
        n = 50 + 7 * f
        fl = rng.random(n)
        fl[:f] = np.nan
        host.append({"env": rng.random(n), "floor": fl, "troughs": np.arange(f, dtype=np.int32),
                     "peaks": np.arange(2 * f, dtype=np.int32) + 1, "flags": f % 3})
    bench.dump_outputs(str(tmp_path / "all"), host, range(10, 16))
    d = _load(tmp_path / "all")
    assert d["sample"].tolist() == list(range(6)) and d["recording_ids"].tolist() == list(range(10, 16))
    assert d["n_troughs"].tolist() == list(range(6)) and d["n_peaks"].tolist() == [2 * f for f in range(6)]
    assert d["flags"].tolist() == [f % 3 for f in range(6)]
    assert np.array_equal(d["env"], np.concatenate([r["env"] for r in host]))
    assert np.array_equal(d["floor"], np.concatenate([r["floor"] for r in host]), equal_nan=True)
    assert np.array_equal(d["peaks"], np.concatenate([r["peaks"] for r in host]))
    assert d["sample_offsets"].tolist() == np.concatenate([[0], np.cumsum([50 + 7 * f for f in range(6)])]).tolist()
    # over the budget: a strict, seeded subset held in full; the counts still cover every recording
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 * 6 * 7 + 3 * 8 * 2 * 90)
    bench.dump_outputs(str(tmp_path / "part"), host, range(6))
    p = _load(tmp_path / "part")
    pick = [int(i) for i in p["sample"]]
    assert 0 < len(pick) < 6 and len(p["n_peaks"]) == 6
    assert np.array_equal(p["env"], np.concatenate([host[i]["env"] for i in pick]))
    assert np.array_equal(p["troughs"], np.concatenate([host[i]["troughs"] for i in pick]))
    assert sum(a.nbytes for a in p.values()) <= bench.DUMP_BUDGET


def test_plain_run_is_lean_and_dumps_repeatably(tmp_path):
    """A plain run reports the headline fields and none of the --full legs; two
    runs with the same arguments dump identical arrays, equal to the oracle's."""
    from oracle import oracle as O
    from bpm_analysis_amd import DEFAULT_PARAMS
    argv = ["--cpu-stub", "--steps", "2", "--warmup", "1", "--files", "2", "--secs", "6"]
    a = _bench(*argv, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*argv, "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
        assert all(line[k] is None for k in FULL_ONLY), {k: line[k] for k in FULL_ONLY if line[k] is not None}
        assert line["unit"] == "audio-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0
        assert abs(line["value"] - 2 * 6 * 44100 / (line["ms_per_step"] / 1e3)) <= 1e-6 * line["value"]
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in DUMP_NAMES:
        assert np.array_equal(da[n], db[n], equal_nan=True), n
    assert a["dumped_outputs"] == {n: int(da[n].size) for n in DUMP_NAMES}
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    outs = [O.detect(O.synth(f, 6 * 44100, 44100, 1), 44100, params, mode="native") for f in range(2)]
    assert da["sample"].tolist() == [0, 1] and da["recording_ids"].tolist() == [0, 1]
    assert np.array_equal(da["env"], np.concatenate([o["env"] for o in outs]))
    assert np.array_equal(da["floor"], np.concatenate([o["floor"] for o in outs]), equal_nan=True)
    assert np.array_equal(da["peaks"], np.concatenate([o["peaks"] for o in outs]))
    assert np.array_equal(da["troughs"], np.concatenate([o["troughs"] for o in outs]))
    assert da["n_peaks"].tolist() == [len(o["peaks"]) for o in outs]


def test_full_run_keeps_the_checks():
    line = _bench("--cpu-stub", "--full", "--steps", "1", "--warmup", "1", "--files", "2", "--secs", "6",
                  "--host-beat-files", "1")
    assert line["full"] is True and line["dumped_outputs"] is None
    assert line["parity"]["ok"] and line["parity"]["files"] == 2
    assert line["cpu_baseline"]["value"] > 0 and line["gpu_vs_cpu"] > 0
    assert line["result_gather"]["files"] == 2 and line["host_beat_stages"]["native"]["files"] == 2


@pytest.mark.gpu
def test_plain_gpu_run_dumps_the_detectors_outputs(tmp_path):
    """On the GPU: the dump of a small plain run equals, bit for bit, what
    Detector.run returns for the same recordings."""
    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd.engine import Detector
    F, secs, fs = 5, 7, 44100
    line = _bench("--steps", "3", "--warmup", "1", "--files", str(F), "--secs", str(secs),
                  "--dump-outputs", str(tmp_path / "d"))
    assert line["full"] is False and line["steps"] == 3 and line["data"] == "synthetic"
    assert all(line[k] is None for k in FULL_ONLY)
    d = _load(tmp_path / "d")
    det = Detector(0)
    fo = np.arange(F + 1, dtype=np.int64) * secs * fs
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    res = det.run(det.synth(fo, fs, 1, seed0=0), fo, fs, params, mode="native").to_host()
    det.close()
    assert d["sample"].tolist() == list(range(F))
    for k in ("env", "floor", "troughs", "peaks"):
        assert np.array_equal(d[k], np.concatenate([r[k] for r in res]).astype(np.float64), equal_nan=True), k
    assert d["flags"].tolist() == [r["flags"] for r in res]
    assert d["n_peaks"].tolist() == [len(r["peaks"]) for r in res] and line["total_raw_peaks"] == sum(d["n_peaks"])
