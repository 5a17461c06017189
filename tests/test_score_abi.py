"""bpmx_score_device without a GPU: the ABI (export, structure field order and
sizes, status, kind, option and record values against the header text, the
argument errors) and the launch plan's LDS / global switch
(tests/score_plan_driver.hip, a host program)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import score_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")
OPT_SCORE_GLOBAL = 262144


def test_export_and_structures():
    assert "bpmx_score_device" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_score_device")
    assert ctypes.sizeof(N.ScoreParams) == 8 and ctypes.sizeof(N.RefMarks) == 32 and ctypes.sizeof(N.ScoreOut) == 48
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry point is additive
    opts = [getattr(N, k) for k in dir(N) if k.startswith("OPT_")]
    assert N.OPT_SCORE_GLOBAL == OPT_SCORE_GLOBAL and opts.count(OPT_SCORE_GLOBAL) == 1
    assert len(set(opts)) == len(opts) and all(v & (v - 1) == 0 for v in opts)
    p = N.ScoreParams(50, 5000)
    assert (p.tol_ms, p.gap_ms) == (50, 5000)


def test_header_and_exports_agree():
    """Every function the header declares is in EXPORTS and in the library, and the other way round."""
    txt = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|const char \*)\s*\*?(bpmx_\w+)\(", txt, re.M))
    assert "bpmx_score_device" in declared
    assert declared == set(N.EXPORTS)
    L = N.load()
    assert all(hasattr(L, name) for name in declared)


def test_header_defines_the_status_option_and_record_values():
    txt = open(HEADER).read()
    assert "#define BPMX_ABI_VERSION 4" in txt
    for name, v in (("BPMX_SCORE_OK", N.SCORE_OK), ("BPMX_SCORE_NO_LABELS", N.SCORE_NO_LABELS),
                    ("BPMX_SCORE_NONE", N.SCORE_NONE), ("BPMX_SCORE_OVERFLOW", N.SCORE_OVERFLOW),
                    ("BPMX_OPT_SCORE_GLOBAL", OPT_SCORE_GLOBAL), ("BPMX_SCORE_OUTSIDE", N.SCORE_OUTSIDE),
                    ("BPMX_SCORE_TP", N.SCORE_TP), ("BPMX_SCORE_SWAP", N.SCORE_SWAP), ("BPMX_SCORE_FP", N.SCORE_FP),
                    ("BPMX_SCORE_FN", N.SCORE_FN), ("BPMX_SR_N_REF", N.SR_N_REF), ("BPMX_SR_N_DET", N.SR_N_DET),
                    ("BPMX_SR_TP", N.SR_TP), ("BPMX_SR_SWAP", N.SR_SWAP), ("BPMX_SR_FP", N.SR_FP),
                    ("BPMX_SR_FN", N.SR_FN), ("BPMX_SR_SUM_ERR", N.SR_SUM_ERR), ("BPMX_SR_SUM_ABS", N.SR_SUM_ABS),
                    ("BPMX_SR_MAX_ABS", N.SR_MAX_ABS), ("BPMX_SR_PER_TYPE", N.SR_PER_TYPE),
                    ("BPMX_SR_N_OUTSIDE", N.SR_N_OUTSIDE), ("BPMX_SR_N_SPANS", N.SR_N_SPANS),
                    ("BPMX_SCORE_RECORD", N.SCORE_RECORD)):
        assert f"{name} = {v}" in txt, name
    assert (N.SCORE_OK, N.SCORE_NO_LABELS, N.SCORE_NONE, N.SCORE_OVERFLOW) == (0, 1, -22, -23)
    assert (N.SCORE_OUTSIDE, N.SCORE_TP, N.SCORE_SWAP, N.SCORE_FP, N.SCORE_FN) == (0, 1, 2, 3, 3)
    assert N.SCORE_RECORD == 20 == 2 * N.SR_PER_TYPE + 2
    from bpm_analysis_amd import _host as H
    codes = {N.SCORE_NONE, N.SCORE_OVERFLOW, N.LABELS_NONE, N.LABELS_OVERFLOW, N.METRICS_NONE, N.METRICS_OVERFLOW,
             N.BEATS_SKIPPED, N.BEATS_OVERFLOW, H.OK, H.E_ARG, H.E_FEW_PEAKS}
    assert len(codes) == 11
    # labels.py states the same numbers
    for k in ("SCORE_OK", "SCORE_NO_LABELS", "SCORE_NONE", "SCORE_OVERFLOW", "SR_N_REF", "SR_N_DET", "SR_TP", "SR_SWAP",
              "SR_FP", "SR_FN", "SR_SUM_ERR", "SR_SUM_ABS", "SR_MAX_ABS", "SR_PER_TYPE", "SR_N_OUTSIDE", "SR_N_SPANS",
              "SCORE_RECORD"):
        assert getattr(LB, k) == getattr(N, k), k
    assert (LB.KIND_OUTSIDE, LB.KIND_TP, LB.KIND_SWAP, LB.KIND_FP, LB.KIND_FN) == \
        (N.SCORE_OUTSIDE, N.SCORE_TP, N.SCORE_SWAP, N.SCORE_FP, N.SCORE_FN)


@pytest.mark.parametrize("struct,cls", [("bpmx_score_params", N.ScoreParams), ("bpmx_ref_marks", N.RefMarks),
                                         ("bpmx_score_out", N.ScoreOut)])
def test_field_order_is_the_bindings(struct, cls):
    txt = open(HEADER).read()
    body = txt[:txt.index("} " + struct + ";")]
    body = body[body.rindex("typedef struct {"):]
    order = [re.search(r"[\s*]" + name + r"[;,]", body).start() for name, _ in cls._fields_]    # the declarators
    assert order == sorted(order)


def _args(tol=50, gap=5000, pk_off=True, rf_off=True):
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)                           # never dereferenced: the arguments are checked first
    sp, pk, lo, rf, o = N.ScoreParams(tol, gap), N.PackedOut(), N.LabelsOut(), N.RefMarks(), N.ScoreOut()
    pk.pk_off = ptr if pk_off else None
    lo.lb_time = lo.lb_type = lo.n_labels = lo.status = ptr
    rf.rf_off = ptr if rf_off else None
    o.record = o.status = ptr
    keep = (one, sp, pk, lo, rf, o)
    return keep, [ctypes.byref(sp), ctypes.byref(pk), ctypes.byref(lo), ctypes.byref(rf), ctypes.byref(o), None]


def test_argument_errors_name_the_entry_point():
    L = N.load()
    ctx = ctypes.c_void_p(1)                              # never dereferenced either
    keep, a = _args()
    assert L.bpmx_score_device(None, 1, *a) == N.E_ARG and b"bpmx_score_device: NULL" in L.bpmx_last_error()
    assert L.bpmx_score_device(ctx, 1, None, *a[1:]) == N.E_ARG and b"bpmx_score_device" in L.bpmx_last_error()
    for tol, gap in ((50, 100), (50, 99), (0, 0), (1000, -5)):
        keep, a = _args(tol, gap)
        assert L.bpmx_score_device(ctx, 1, *a) == N.E_ARG
        assert b"bpmx_score_device: needs gap_ms > 2 * tol_ms" in L.bpmx_last_error(), (tol, gap)
    keep, a = _args(-1, 5000)
    assert L.bpmx_score_device(ctx, 1, *a) == N.E_ARG and b"bpmx_score_device: needs tol_ms >= 0" in L.bpmx_last_error()
    keep, a = _args(rf_off=False)
    assert L.bpmx_score_device(ctx, 1, *a) == N.E_ARG and b"bpmx_score_device: needs rf_off" in L.bpmx_last_error()
    keep, a = _args(pk_off=False)
    assert L.bpmx_score_device(ctx, 1, *a) == N.E_ARG and b"bpmx_score_device: needs pk_off" in L.bpmx_last_error()
    keep, a = _args()
    assert L.bpmx_score_device(ctx, -1, *a) == N.E_ARG and b"n_files" in L.bpmx_last_error()
    keep[5].sc_kind = ctypes.addressof(keep[0])           # one row pointer of the four
    assert L.bpmx_score_device(ctx, 1, *a) == N.E_ARG and b"together" in L.bpmx_last_error()


def test_no_files_is_ok():
    L = N.load()
    keep, a = _args()
    assert L.bpmx_score_device(ctypes.c_void_p(1), 0, *a) == N.OK
    keep, a = _args(50, 100)                              # the parameters are checked all the same
    assert L.bpmx_score_device(ctypes.c_void_p(1), 0, *a) == N.E_ARG


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "score_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_structure_sizes_match_the_binding(plan):
    sizes, = plan()
    assert sizes["sizeof_params"] == ctypes.sizeof(N.ScoreParams)
    assert sizes["sizeof_ref"] == ctypes.sizeof(N.RefMarks)
    assert sizes["sizeof_out"] == ctypes.sizeof(N.ScoreOut)
    assert sizes["record"] == N.SCORE_RECORD and sizes["threads"] == 256
    # a global slice holds a recording's workspace whatever its offsets: the per-mark arrays and the rounding to 8
    assert sizes["stride"] >= max(sizes["per_det"], sizes["per_ref"]) and sizes["stride"] % 8 == 0


def test_plan_switches_at_the_lds_budget(plan):
    sizes, p0 = plan("1:605:605:0")
    limit, budget = p0["max_n"], p0["budget"]
    # five workgroups in a CU's 160 KB, and a 60 s recording's most labels with as many reference marks fit
    assert 5 * budget <= 160 * 1024 and p0["bytes"] <= budget and limit >= 605
    assert (p0["lds"], p0["any_global"], p0["gws"], p0["grid"]) == (p0["bytes"], 0, 0, 1)
    _, at, over, wide, forced, empty = plan(f"4:{limit}:{limit}:0", f"4:{limit + 8}:{limit + 8}:0",
                                            f"1024:{1024 * 605}:{1024 * 605}:0", f"4:{limit}:{limit}:{OPT_SCORE_GLOBAL}",
                                            "3:0:0:0")
    assert at["bytes"] <= budget < over["bytes"]
    assert (at["lds"], at["any_global"], at["gws"], at["grid"]) == (at["bytes"], 0, 0, 4)
    assert (over["lds"], over["any_global"]) == (budget, 1)
    assert over["gws"] == 4 * over["fixed"] + (2 * limit + 16) * sizes["stride"]
    assert (wide["grid"], wide["lds"], wide["any_global"]) == (1024, budget, 1)
    assert (forced["lds"], forced["any_global"]) == (0, 1) and forced["gws"] == 4 * forced["fixed"] + 2 * limit * sizes["stride"]
    assert (empty["lds"], empty["any_global"], empty["gws"]) == (empty["head"], 0, 0)
    assert at["fixed"] >= at["head"] + 16 * sizes["stride"] - 8
    # the shared cases hold one count beyond the budget on both sides, and the largest count within it
    assert SC.OVER > limit > max(SC.COUNTS)
