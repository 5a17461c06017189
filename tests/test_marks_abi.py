"""bpmx_marks_device without a GPU: the ABI (export, structure field order and
sizes, status, option and record values against the header text, the argument
errors, n_files = 0) and the launch plan's LDS / global switch
(tests/marks_plan_driver.hip, a host program)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import marks_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")
OPT_MARKS_GLOBAL = 524288


def test_export_and_structures():
    assert "bpmx_marks_device" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_marks_device")
    assert ctypes.sizeof(N.MarksParams) == 8 and ctypes.sizeof(N.RefMarks) == 32
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry point is additive
    opts = [getattr(N, k) for k in dir(N) if k.startswith("OPT_")]
    assert N.OPT_MARKS_GLOBAL == OPT_MARKS_GLOBAL and opts.count(OPT_MARKS_GLOBAL) == 1
    assert len(set(opts)) == len(opts) and all(v & (v - 1) == 0 for v in opts)
    assert N.MarksParams(2.5).smoothing_window_sec == 2.5


def test_header_and_exports_agree():
    """Every function the header declares is in EXPORTS and in the library, and the other way round."""
    txt = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|const char \*)\s*\*?(bpmx_\w+)\(", txt, re.M))
    assert "bpmx_marks_device" in declared
    assert declared == set(N.EXPORTS)
    L = N.load()
    assert all(hasattr(L, name) for name in declared)
    note = txt[:txt.index("#define BPMX_ABI_VERSION")][-400:]
    assert "bpmx_marks_device" in note and "BPMX_OPT_MARKS_GLOBAL" in note


def test_header_defines_the_status_option_and_record_values():
    txt = open(HEADER).read()
    assert "#define BPMX_ABI_VERSION 4" in txt
    for name, v in (("BPMX_MARKS_FEW", N.MARKS_FEW), ("BPMX_MARKS_OVERFLOW", N.MARKS_OVERFLOW),
                    ("BPMX_OPT_MARKS_GLOBAL", OPT_MARKS_GLOBAL), ("BPMX_MK_N_ROWS", N.MK_N_ROWS),
                    ("BPMX_MK_N_S1", N.MK_N_S1), ("BPMX_MK_N_S2", N.MK_N_S2), ("BPMX_MK_N_MERGED", N.MK_N_MERGED),
                    ("BPMX_MK_N_DROPPED", N.MK_N_DROPPED), ("BPMX_MK_N_OTHER", N.MK_N_OTHER),
                    ("BPMX_MARKS_RECORD", N.MARKS_RECORD)):
        assert f"{name} = {v}" in txt, name
    assert (N.MARKS_FEW, N.MARKS_OVERFLOW, N.MARKS_RECORD) == (-24, -25, 8)
    assert (N.MK_N_ROWS, N.MK_N_S1, N.MK_N_S2, N.MK_N_MERGED, N.MK_N_DROPPED, N.MK_N_OTHER) == (0, 1, 2, 3, 4, 5)
    # distinct from every other code, in the bindings and in the header's text
    codes = [N.MARKS_FEW, N.MARKS_OVERFLOW, N.SCORE_NONE, N.SCORE_OVERFLOW, N.LABELS_NONE, N.LABELS_OVERFLOW,
             N.METRICS_NONE, N.METRICS_OVERFLOW, N.BEATS_SKIPPED, N.BEATS_OVERFLOW, H.OK, H.E_ARG, H.E_FEW_PEAKS]
    assert len(set(codes)) == len(codes)
    neg = [int(v) for v in re.findall(r"\bBPMX_\w+\s*=\s*(-\d+)", txt)]
    assert neg.count(-24) == 1 and neg.count(-25) == 1
    bits = [int(v) for v in re.findall(r"\bBPMX_OPT_\w+\s*=\s*(\d+)", txt)]
    assert bits.count(OPT_MARKS_GLOBAL) == 1 and len(set(bits)) == len(bits)
    # labels.py states the same numbers
    for k in ("MARKS_FEW", "MARKS_OVERFLOW", "MK_N_ROWS", "MK_N_S1", "MK_N_S2", "MK_N_MERGED", "MK_N_DROPPED",
              "MK_N_OTHER", "MARKS_RECORD"):
        assert getattr(LB, k) == getattr(N, k), k
    assert (LB.S1, LB.S2) == (N.LABEL_S1, N.LABEL_S2) == (1, 2)          # bpmx_beat_tag's S1 / S2 too


@pytest.mark.parametrize("struct,cls", [("bpmx_marks_params", N.MarksParams), ("bpmx_ref_marks", N.RefMarks),
                                         ("bpmx_packed", N.PackedOut), ("bpmx_beats_out", N.BeatsOut)])
def test_field_order_is_the_bindings(struct, cls):
    txt = open(HEADER).read()
    body = txt[:txt.index("} " + struct + ";")]
    body = body[body.rindex("typedef struct {"):]
    names = [n.rstrip("_") for n, _ in cls._fields_]
    order = [re.search(r"[\s*]" + n + r"[;,]", body).start() for n in names]    # the declarators
    assert order == sorted(order)


def _args(window=5.0, rf_off=True, pk_off=True, final=True):
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)                           # never dereferenced: the arguments are checked first
    mp, rf, pk, bo = N.MarksParams(window), N.RefMarks(), N.PackedOut(), N.BeatsOut()
    rf.rf_off = ptr if rf_off else None
    pk.pk_off = ptr if pk_off else None
    pk.pk_idx = ptr
    bo.final_idx = ptr if final else None
    bo.n_final = bo.bpm_t = bo.bpm = bo.n_bpm = bo.tags = bo.status = ptr
    keep = (one, mp, rf, pk, bo)
    return keep, [ctypes.byref(mp), ctypes.byref(rf), None, ctypes.byref(pk), ctypes.byref(bo), ptr, ptr, None]


def test_argument_errors_name_the_entry_point():
    L = N.load()
    ctx = ctypes.c_void_p(1)                              # never dereferenced either
    err = lambda: L.bpmx_last_error()  # noqa: E731
    keep, a = _args()
    assert L.bpmx_marks_device(None, 1, 147, *a) == N.E_ARG and b"bpmx_marks_device: NULL" in err()
    assert L.bpmx_marks_device(ctx, 1, 147, None, *a[1:]) == N.E_ARG and b"bpmx_marks_device: NULL" in err()
    for k in (1, 3, 4, 5, 6):                             # marks, tables, beats, gap, record
        b = list(a)
        b[k] = None
        assert L.bpmx_marks_device(ctx, 1, 147, *b) == N.E_ARG and b"bpmx_marks_device: NULL" in err(), k
    for sr in (0, -1):
        assert L.bpmx_marks_device(ctx, 1, sr, *a) == N.E_ARG and b"bpmx_marks_device: bad n_files/sr" in err()
    assert L.bpmx_marks_device(ctx, -1, 147, *a) == N.E_ARG and b"bpmx_marks_device: bad n_files/sr" in err()
    for w in (0.0, -1.0, float("nan")):
        keep, a = _args(window=w)
        assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG
        assert b"bpmx_marks_device: needs smoothing_window_sec > 0" in err(), w
    keep, a = _args(rf_off=False)
    assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"bpmx_marks_device: needs rf_off" in err()
    keep, a = _args()
    keep[2].cap_ref = 3                                   # marks without rf_ms / rf_type
    assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"bpmx_marks_device: needs rf_off" in err()
    keep[2].cap_ref = 2 ** 31 - 1
    assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"cap_ref < 2^31" in err()
    keep, a = _args(pk_off=False)
    assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"bpmx_marks_device: needs pk_off" in err()
    keep, a = _args()
    for cap in (2 ** 31 - 1, 2 ** 31, -1):
        keep[3].cap_peaks = cap
        assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"cap_peaks < 2^31" in err(), cap
    keep, a = _args(final=False)
    assert L.bpmx_marks_device(ctx, 1, 147, *a) == N.E_ARG and b"bpmx_marks_device: the beats' final_idx" in err()


def test_no_files_is_ok():
    L = N.load()
    keep, a = _args()
    assert L.bpmx_marks_device(ctypes.c_void_p(1), 0, 147, *a) == N.OK
    keep, a = _args(rf_off=False, pk_off=False, final=False)      # nothing of the tables is looked at
    assert L.bpmx_marks_device(ctypes.c_void_p(1), 0, 147, *a) == N.OK
    keep, a = _args(window=0.0)                           # the parameters are checked all the same
    assert L.bpmx_marks_device(ctypes.c_void_p(1), 0, 147, *a) == N.E_ARG


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("marks_plan") / "marks_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "marks_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_structure_sizes_match_the_binding(plan):
    sizes, = plan()
    assert sizes["sizeof_params"] == ctypes.sizeof(N.MarksParams)
    assert sizes["sizeof_ref"] == ctypes.sizeof(N.RefMarks)
    assert sizes["sizeof_packed"] == ctypes.sizeof(N.PackedOut)
    assert sizes["sizeof_beats"] == ctypes.sizeof(N.BeatsOut)
    assert sizes["record"] == N.MARKS_RECORD == sizes["per_file"] and sizes["threads"] == 256
    # a global slice holds a recording's workspace whatever its offset: the per-beat arrays and the rounding to 8
    assert sizes["stride"] >= sizes["per_s1"] and sizes["stride"] % 8 == 0


def test_plan_switches_at_the_lds_budget(plan):
    sizes, p0 = plan("1:605:0")
    limit, budget = p0["max_n"], p0["budget"]
    # five workgroups in a CU's 160 KB, and the most beats of a 60 s recording fit
    assert 5 * budget <= 160 * 1024 and p0["bytes"] <= budget and limit >= 605
    assert (p0["lds_n"], p0["lds"], p0["any_global"], p0["gws"], p0["grid"]) == (605, p0["bytes"], 0, 0, 1)
    _, at, over, wide, forced, empty, forced_empty = plan(f"4:{limit}:0", f"4:{limit + 8}:0", f"1024:{1024 * 605}:0",
                                                          f"4:{limit}:{OPT_MARKS_GLOBAL}", "3:0:0",
                                                          f"3:0:{OPT_MARKS_GLOBAL}")
    assert at["bytes"] <= budget < over["bytes"]
    assert (at["lds_n"], at["lds"], at["any_global"], at["gws"], at["grid"]) == (limit, at["bytes"], 0, 0, 4)
    assert (over["lds_n"], over["lds"], over["any_global"]) == (limit, at["bytes"], 1)
    assert over["gws"] == 4 * over["fixed"] + (limit + 8) * sizes["stride"]
    assert (wide["grid"], wide["lds_n"], wide["any_global"]) == (1024, limit, 1)
    assert (forced["lds_n"], forced["lds"], forced["any_global"]) == (-1, 0, 1)
    assert forced["gws"] == 4 * forced["fixed"] + limit * sizes["stride"]
    assert (empty["lds_n"], empty["lds"], empty["any_global"], empty["gws"]) == (0, empty["bytes"], 0, 0)
    assert (forced_empty["lds_n"], forced_empty["any_global"], forced_empty["gws"]) == (-1, 1, 3 * forced_empty["fixed"])
    # a slice of f * fixed + stride * rf_off[f] holds the workspace of as many S1 rows as the recording has marks
    assert at["fixed"] >= at["head"] + 128 + 7 * sizes["stride"]
    for n in (0, 1, 7, 8, 9, limit + 8):
        assert plan(f"1:{n}:0")[1]["bytes"] <= at["fixed"] + n * sizes["stride"], n
    # the row scratch: four arrays of cap_ref entries behind one another, then the counts
    for p, ref, F in ((at, limit, 4), (over, limit + 8, 4), (empty, 0, 3)):
        c8 = (ref + 7) // 8 * 8
        assert (p["o_ridx"], p["o_ktype"], p["o_rtag"], p["o_cnt"]) == (4 * c8, 8 * c8, 9 * c8, 10 * c8)
        assert p["rows"] == 10 * c8 + F * sizes["per_file"] * 4 and sizes["scratch"] == 10
    # the shared cases hold S1 counts at the limit and one step beyond it
    assert MC.LIMIT == limit and 700 // 2 < limit
