"""bpmx_beats_device without a GPU: the ABI (export, structure size, version),
the launch plan's LDS / global switch (tests/beats_plan_driver.hip, a host
program) and shard.run_sharded(beats="device") on CPU doubles that have no
device stage, which must behave exactly as beats="native"."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
OPT_BEATS_GLOBAL = 16384


def test_export_and_structure():
    assert "bpmx_beats_device" in N.EXPORTS and "bpmx_set_options" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_beats_device") and hasattr(L, "bpmx_set_options")
    assert ctypes.sizeof(N.BeatsOut) == 8 * 8
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4
    assert N.OPT_BEATS_GLOBAL == OPT_BEATS_GLOBAL
    # the new status values stay clear of the host library's
    assert len({N.BEATS_SKIPPED, N.BEATS_OVERFLOW, H.OK, H.E_ARG, H.E_FEW_PEAKS}) == 5


def test_header_defines_the_status_values_and_includes_the_host_header():
    txt = open(os.path.join(os.path.dirname(HERE), "include", "bpmx.h")).read()
    assert '#include "bpmx_host.h"' in txt
    assert f"BPMX_BEATS_SKIPPED = {N.BEATS_SKIPPED}" in txt and f"BPMX_BEATS_OVERFLOW = {N.BEATS_OVERFLOW}" in txt
    assert "#define BPMX_ABI_VERSION 4" in txt


def test_null_arguments_are_argument_errors():
    L = N.load()
    rc = L.bpmx_beats_device(None, 1, 302, None, 0.0, None, None, None, None)
    assert rc == N.E_ARG and b"bpmx_beats_device" in L.bpmx_last_error()
    assert L.bpmx_set_options(None, 0) == N.E_ARG


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("beats_plan") / "beats_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "beats_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_plan_switches_at_the_lds_limit(plan):
    p0, = plan("1:605:0")
    limit, budget = p0["max_peaks"], p0["budget"]
    # a quarter of the CU's 160 KB, and the most peaks of a 60 s recording fit
    assert 4 * budget <= 160 * 1024 and p0["bytes_605"] <= budget and limit >= 605
    at, over, bench, one, forced = plan(f"4:{limit}:0", f"4:{limit + 1}:0", f"1024:{1024 * 605}:0", "1:605:0",
                                        f"4:{limit}:{OPT_BEATS_GLOBAL}")
    assert (at["lds_n"], at["any_global"], at["gws"]) == (limit, 0, 0) and at["lds"] <= budget
    assert (over["lds_n"], over["any_global"]) == (limit, 1) and over["lds"] == at["lds"]
    assert over["gws"] == 4 * over["fixed"] + (limit + 1) * over["stride"]
    assert (bench["grid"], one["grid"]) == (1024, 1)
    assert bench["lds_n"] == limit and bench["lds"] <= budget
    assert (one["lds_n"], one["any_global"]) == (605, 0) and one["lds"] == one["bytes_605"]
    assert (forced["lds_n"], forced["lds"], forced["any_global"]) == (-1, 0, 1) and forced["gws"] > 0


def test_run_sharded_device_falls_back_to_native_without_the_stage():
    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd.shard import run_sharded
    from oracle import oracle as O
    from tests.test_packed_host import _FullDouble, _PackedDouble
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    items = [O.synth(60 + i, n, 44100, 1) for i, n in enumerate([44100 * 9, 44100 * 14 + 3, 146 * 15, 44100 * 11])]
    kw = dict(fs=44100, mode="native", host_threads=2, chunk_frames=44100 * 20)
    for double in (_PackedDouble, _FullDouble):
        da, db = double(), double()
        assert not hasattr(da, "run_host_beats")
        a = run_sharded(items, params, detector=da, beats="native", **kw)
        b = run_sharded(items, params, detector=db, beats="device", **kw)
        assert da.calls == db.calls and len(a) == len(b) == len(items)
        for x, y in zip(a, b):
            assert sorted(x) == sorted(y)
            for k, v in x.items():
                if k == "error":
                    assert type(v) is type(y[k]) and str(v) == str(y[k])
                elif isinstance(v, np.ndarray):
                    assert v.dtype == y[k].dtype and np.array_equal(v, y[k], equal_nan=True), k
                else:
                    assert v == y[k], k
        assert len(a[0]["final_peaks"]) > 2
