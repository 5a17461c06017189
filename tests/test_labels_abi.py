"""bpmx_labels_device without a GPU: the ABI (export, structure sizes, status,
option and record values against the header text, null arguments) and the
launch plan's LDS / global switch (tests/labels_plan_driver.hip, a host
program)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from bpm_analysis_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")
OPT_LABELS_GLOBAL = 131072


def test_export_and_structures():
    assert "bpmx_labels_device" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_labels_device")
    assert ctypes.sizeof(N.LabelParams) == 8 and ctypes.sizeof(N.LabelsOut) == 19 * 8
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry point is additive
    opts = [getattr(N, k) for k in dir(N) if k.startswith("OPT_")]
    assert N.OPT_LABELS_GLOBAL == OPT_LABELS_GLOBAL and opts.count(OPT_LABELS_GLOBAL) == 1
    assert len(set(opts)) == len(opts) and all(v & (v - 1) == 0 for v in opts)
    assert N.LabelParams(5.0).gap_sec == 5.0


def test_header_defines_the_status_option_and_record_values():
    txt = open(HEADER).read()
    assert "#define BPMX_ABI_VERSION 4" in txt
    for name, v in (("BPMX_LABELS_OK", N.LABELS_OK), ("BPMX_LABELS_NONE", N.LABELS_NONE),
                    ("BPMX_LABELS_OVERFLOW", N.LABELS_OVERFLOW), ("BPMX_OPT_LABELS_GLOBAL", OPT_LABELS_GLOBAL),
                    ("BPMX_LABEL_S1", N.LABEL_S1), ("BPMX_LABEL_S2", N.LABEL_S2), ("BPMX_LR_AVG_DT", N.LR_AVG_DT),
                    ("BPMX_LR_AVG_BPM", N.LR_AVG_BPM), ("BPMX_LR_N_S1", N.LR_N_S1), ("BPMX_LR_N_S2", N.LR_N_S2),
                    ("BPMX_LABELS_RECORD", N.LABELS_RECORD)):
        assert f"{name} = {v}" in txt, name
    from bpm_analysis_amd import _host as H
    codes = {N.LABELS_NONE, N.LABELS_OVERFLOW, N.METRICS_NONE, N.METRICS_OVERFLOW, N.BEATS_SKIPPED, N.BEATS_OVERFLOW,
             H.OK, H.E_ARG, H.E_FEW_PEAKS}
    assert len(codes) == 9
    # the field order of bpmx_labels_out is the binding's
    body = txt[txt.index("enum bpmx_labels_record"):]
    body = body[body.index("typedef struct {"):body.index("} bpmx_labels_out;")]
    order = [body.index("*" + name) for name, _ in N.LabelsOut._fields_]          # the declarators
    assert order == sorted(order)
    from bpm_analysis_amd import labels as LB
    assert (LB.S1, LB.S2) == (N.LABEL_S1, N.LABEL_S2)


def test_null_arguments_are_argument_errors():
    L = N.load()
    rc = L.bpmx_labels_device(None, 1, 302, None, None, None, None, None, None)
    assert rc == N.E_ARG and b"bpmx_labels_device" in L.bpmx_last_error()
    # the trace's gap labels are a required input: everything else set, gap NULL
    ctx = ctypes.c_void_p(1)                              # never dereferenced: the arguments are checked first
    lp, pk, b, o = N.LabelParams(5.0), N.PackedOut(), N.BeatsOut(), N.LabelsOut()
    rc = L.bpmx_labels_device(ctx, 1, 302, ctypes.byref(lp), ctypes.byref(pk), ctypes.byref(b), None,
                              ctypes.byref(o), None)
    assert rc == N.E_ARG and b"gap" in L.bpmx_last_error()
    gap = ctypes.c_int32(0)
    rc = L.bpmx_labels_device(ctx, 1, 302, ctypes.byref(lp), ctypes.byref(pk), ctypes.byref(b),
                              ctypes.addressof(gap), ctypes.byref(o), None)
    assert rc == N.E_ARG and b"bpmx_labels_device: needs pk_off" in L.bpmx_last_error()
    rc = L.bpmx_labels_device(ctx, 0, 302, ctypes.byref(lp), ctypes.byref(pk), ctypes.byref(b),
                              ctypes.addressof(gap), ctypes.byref(o), None)
    assert rc == N.E_ARG and b"n_files" in L.bpmx_last_error()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("labels_plan") / "labels_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "labels_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_structure_sizes_match_the_binding(plan):
    sizes, = plan()
    assert sizes["sizeof_params"] == ctypes.sizeof(N.LabelParams)
    assert sizes["sizeof_out"] == ctypes.sizeof(N.LabelsOut)
    assert sizes["record"] == N.LABELS_RECORD and sizes["threads"] == 256


def test_plan_switches_at_the_lds_limit(plan):
    _, p0 = plan("1:605:0")
    limit, budget = p0["max_n"], p0["budget"]
    # four workgroups in a CU's 160 KB, and the most peaks of a 60 s recording fit
    assert 4 * budget <= 160 * 1024 and p0["bytes_605"] <= budget and limit >= 605
    _, at, over, bench, one, forced = plan(f"4:{limit}:0", f"4:{limit + 1}:0", f"1024:{1024 * 605}:0", "1:605:0",
                                           f"4:{limit}:{OPT_LABELS_GLOBAL}")
    assert (at["lds_n"], at["any_global"], at["gws"]) == (limit, 0, 0) and at["lds"] <= budget
    assert (over["lds_n"], over["any_global"]) == (limit, 1) and over["lds"] == at["lds"]
    assert over["gws"] == 4 * over["fixed"] + (limit + 1) * over["stride"]
    assert (bench["grid"], one["grid"], at["grid"]) == (1024, 1, 4)
    assert bench["lds_n"] == limit and bench["lds"] <= budget
    assert (one["lds_n"], one["any_global"]) == (605, 0) and one["lds"] == one["bytes_605"]
    assert (forced["lds_n"], forced["lds"], forced["any_global"]) == (-1, 0, 1) and forced["gws"] > 0
    # a global slice holds a recording's workspace whatever its offset: the per-peak arrays and the rounding to 8
    _, p = plan("1:605:0")
    sizes, = plan()
    assert p["stride"] >= sizes["per"]
