"""bpmx_metrics_device without a GPU: the ABI (export, structure sizes, status
and option values against the header text, null arguments), the launch plan's
LDS / global switch (tests/metrics_plan_driver.hip, a host program) and
shard.run_sharded(metrics=True) on CPU doubles that have no device stage,
which must fall back to the host's final_metrics and equal it."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")
OPT_METRICS_GLOBAL = 32768


def test_export_and_structures():
    assert "bpmx_metrics_device" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_metrics_device")
    assert ctypes.sizeof(N.MetricParams) == 48 and ctypes.sizeof(N.MetricsOut) == 17 * 8
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry point is additive
    assert N.OPT_METRICS_GLOBAL == OPT_METRICS_GLOBAL and N.OPT_METRICS_GLOBAL != N.OPT_BEATS_GLOBAL
    p = N.metric_params({"hrv_window_size_beats": 40, "hrv_step_size_beats": 5})
    assert (p.hrv_window_size_beats, p.hrv_step_size_beats) == (40, 5)
    assert (p.min_duration_sec, p.min_bpm_change, p.prominence, p.slope_window_sec, p.hrr_interval_sec) == \
        (10.0, 15.0, 5.0, 20.0, 60.0)


def test_header_defines_the_status_option_and_record_values():
    txt = open(HEADER).read()
    assert "#define BPMX_ABI_VERSION 4" in txt
    for name, v in (("BPMX_METRICS_OK", N.METRICS_OK), ("BPMX_METRICS_TIE", N.METRICS_TIE),
                    ("BPMX_METRICS_E_DISTANCE", N.METRICS_E_DISTANCE), ("BPMX_METRICS_NONE", N.METRICS_NONE),
                    ("BPMX_METRICS_OVERFLOW", N.METRICS_OVERFLOW), ("BPMX_OPT_METRICS_GLOBAL", OPT_METRICS_GLOBAL),
                    ("BPMX_MR_AVG_BPM", N.MR_AVG_BPM), ("BPMX_MR_MIN_BPM", N.MR_MIN_BPM),
                    ("BPMX_MR_MAX_BPM", N.MR_MAX_BPM), ("BPMX_MR_AVG_RMSSDC", N.MR_AVG_RMSSDC),
                    ("BPMX_MR_AVG_SDNN", N.MR_AVG_SDNN), ("BPMX_MR_HRR_PEAK", N.MR_HRR_PEAK),
                    ("BPMX_MR_HRR_RECOVERY_BPM", N.MR_HRR_RECOVERY_BPM), ("BPMX_MR_HRR_VALUE", N.MR_HRR_VALUE),
                    ("BPMX_MR_RECOVERY", N.MR_RECOVERY), ("BPMX_MR_EXERTION", N.MR_EXERTION),
                    ("BPMX_METRICS_RECORD", N.METRICS_RECORD)):
        assert f"{name} = {v}" in txt, name
    from bpm_analysis_amd import _host as H
    codes = {N.METRICS_NONE, N.METRICS_OVERFLOW, N.BEATS_SKIPPED, N.BEATS_OVERFLOW, H.OK, H.E_ARG, H.E_FEW_PEAKS}
    assert len(codes) == 7
    # the field order of bpmx_metrics_out is the binding's
    body = txt[txt.index("typedef struct {            /* device; per-file slices start at pk_off[f] (rows"):]
    body = body[:body.index("} bpmx_metrics_out;")]
    order = [body.index(name) for name, _ in N.MetricsOut._fields_]
    assert order == sorted(order)


def test_null_arguments_are_argument_errors():
    L = N.load()
    rc = L.bpmx_metrics_device(None, 1, 302, None, 0, None, None, None, None)
    assert rc == N.E_ARG and b"bpmx_metrics_device" in L.bpmx_last_error()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("metrics_plan") / "metrics_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "metrics_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_structure_sizes_match_the_binding(plan):
    sizes, = plan()
    assert sizes["sizeof_params"] == ctypes.sizeof(N.MetricParams)
    assert sizes["sizeof_out"] == ctypes.sizeof(N.MetricsOut)
    assert sizes["sizeof_frame"] == 24 and sizes["record"] == N.METRICS_RECORD


def test_plan_switches_at_the_lds_limit(plan):
    _, p0 = plan("1:605:0:40")
    limit, budget = p0["max_n"], p0["budget"]
    # three workgroups in a CU's 160 KB, and the most peaks of a 60 s recording fit
    assert 3 * budget <= 160 * 1024 and p0["bytes_605"] <= budget and limit >= 605 and p0["fw"] == 0
    _, at, over, bench, one, forced = plan(f"4:{limit}:0:40", f"4:{limit + 1}:0:40", f"1024:{1024 * 605}:0:40",
                                           "1:605:0:40", f"4:{limit}:{OPT_METRICS_GLOBAL}:40")
    assert (at["lds_n"], at["any_global"], at["gws"]) == (limit, 0, 0) and at["lds"] <= budget
    assert (over["lds_n"], over["any_global"]) == (limit, 1) and over["lds"] == at["lds"]
    assert over["gws"] == 4 * over["fixed"] + (limit + 1) * over["stride"]
    assert (bench["grid"], one["grid"], at["grid"]) == (1024, 1, 4)
    assert bench["lds_n"] == limit and bench["lds"] <= budget
    assert (one["lds_n"], one["any_global"]) == (605, 0) and one["lds"] == one["bytes_605"]
    assert (forced["lds_n"], forced["lds"], forced["any_global"]) == (-1, 0, 1) and forced["gws"] > 0


def test_plan_gives_the_window_sums_their_stacks(plan):
    """A window of more than 128 beats needs a pairwise-sum stack per thread,
    which comes out of the LDS budget."""
    _, w128, w129, w4096 = plan("4:605:0:128", "4:605:0:129", "4:605:0:4096")
    assert w128["fw"] == 0 and 0 < w129["fw"] <= w4096["fw"]
    assert w129["max_n"] < w128["max_n"] and w129["lds"] <= w129["budget"]
    assert w129["fixed"] > w128["fixed"]
    assert w129["lds_n"] == min(605, w129["max_n"]) and w129["any_global"] == (w129["lds_n"] < 605)
    # at 4096 beats the stacks alone exceed the budget: every recording works in global memory
    assert (w4096["lds_n"], w4096["lds"], w4096["any_global"]) == (-1, 0, 1) and w4096["gws"] > 0


def test_run_sharded_metrics_falls_back_to_the_host():
    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import beats as B
    from bpm_analysis_amd import metrics as MH
    from bpm_analysis_amd.shard import run_sharded
    from oracle import oracle as O
    from tests.test_packed_host import _FullDouble, _PackedDouble
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    items = [O.synth(60 + i, n, 44100, 1) for i, n in enumerate([44100 * 9, 44100 * 14 + 3, 146 * 15, 44100 * 11])]
    kw = dict(fs=44100, mode="native", host_threads=2, chunk_frames=44100 * 20)
    for double in (_PackedDouble, _FullDouble):
        for beats in ("device", "native", "python"):
            da, db = double(), double()
            assert not hasattr(da, "run_host_metrics")
            a = run_sharded(items, params, detector=da, beats=beats, **kw)
            b = run_sharded(items, params, detector=db, beats=beats, metrics=True, **kw)
            assert da.calls == db.calls and len(a) == len(b) == len(items)
            n = 0
            for x, y in zip(a, b):
                # everything the default returns is unchanged
                assert sorted(y) == sorted(list(x) + ([] if "error" in x else ["metrics_record", "n_hrv"]))
                for k, v in x.items():
                    if k == "error":
                        assert type(v) is type(y[k]) and str(v) == str(y[k])
                    elif isinstance(v, np.ndarray):
                        assert v.dtype == y[k].dtype and v.tobytes() == y[k].tobytes(), k
                    else:
                        assert v == y[k], k
                if "error" in x:
                    continue
                m = B.final_metrics(x["final_peaks"], 302, params) if len(x["final_peaks"]) >= 2 else None
                rec, nh = MH.record_of(m)
                assert y["metrics_record"].dtype == np.float64 and y["metrics_record"].shape == (N.METRICS_RECORD,)
                assert y["metrics_record"].tobytes() == rec.tobytes() and y["n_hrv"] == nh
                assert m is None or (rec[N.MR_AVG_BPM] == m["hrv_summary"]["avg_bpm"]
                                     and rec[N.MR_MAX_BPM] == m["smoothed_bpm"].max())
                n += m is not None
            assert n >= 2
