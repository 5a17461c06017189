"""bpmx_hrvspec_device without a GPU: the ABI (exports, structure field order
and sizes against the header text, the option bit, the status values, the
version), the window count at its edges, every argument error, and the LDS
limit through the host driver (tests/hrvspec_core_driver.cpp in its ``plan``
mode)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import hrv_spectrum as HS

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")


def test_exports_and_structures():
    assert "bpmx_hrvspec_device" in N.EXPORTS and "bpmx_hrvspec_windows" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_hrvspec_device") and hasattr(L, "bpmx_hrvspec_windows")
    assert ctypes.sizeof(N.HrvspecParams) == 72 and ctypes.sizeof(N.HrvspecOut) == 88
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry points are additive
    opts = [getattr(N, k) for k in dir(N) if k.startswith("OPT_")]
    assert len(set(opts)) == len(opts) and all(v & (v - 1) == 0 for v in opts)
    p = N.hrvspec_params(HS.geometry(302))
    assert (p.win, p.hop, p.dmin, p.dmax, p.min_intervals, p.min_span, p.n_freq) == (36240, 9060, 76, 453, 16, 7550, 256)
    assert (p.lf_a, p.lf_b, p.hf_a, p.hf_b, p.reserved) == (0, 78, 78, 256, 0) and p.om0 > 0 and p.dom > 0


def test_header_and_exports_agree():
    txt = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|const char \*)\s*\*?(bpmx_\w+)\(", txt, re.M))
    assert {"bpmx_hrvspec_device", "bpmx_hrvspec_windows"} <= declared
    assert declared == set(N.EXPORTS)
    assert "#define BPMX_ABI_VERSION 4" in txt
    note = txt[:txt.index("#define BPMX_ABI_VERSION")][-400:]
    assert "bpmx_hrvspec_device" in note and "bpmx_hrvspec_windows" in note and "BPMX_OPT_HRVSPEC_DIRECT" in note
    added = note[note.index("bpmx_tempo_device") + len("bpmx_tempo_device"):]
    assert len(added) <= 150
    bits = [int(v) for v in re.findall(r"\bBPMX_OPT_\w+\s*=\s*(\d+)", txt)]
    assert len(set(bits)) == len(bits) and all(v & (v - 1) == 0 for v in bits)
    assert sorted(bits) == sorted(getattr(N, k) for k in dir(N) if k.startswith("OPT_"))
    # both forms of the kernel were kept: the rotation along the grid is the default, the other is behind the bit
    assert re.search(r"BPMX_OPT_HRVSPEC_DIRECT\s*=\s*2097152\b", txt) and N.OPT_HRVSPEC_DIRECT == 2097152
    assert max(bits) == 2097152
    for name, v in (("OK", 0), ("NONE", -26), ("OVERFLOW", -27)):
        assert re.search(r"BPMX_HRVSPEC_%s\s*=\s*%d\b" % (name, v), txt), name
        assert getattr(N, "HRVSPEC_" + name) == v == getattr(HS, name)
    assert re.search(r"BPMX_HRVSPEC_RECORD\s*=\s*8\b", txt) and N.HRVSPEC_RECORD == 8 == HS.RECORD


@pytest.mark.parametrize("struct,cls", [("bpmx_hrvspec_params", N.HrvspecParams), ("bpmx_hrvspec_out", N.HrvspecOut)])
def test_field_order_is_the_bindings(struct, cls):
    txt = open(HEADER).read()
    body = txt[:txt.index("} " + struct + ";")]
    body = body[body.rindex("typedef struct {"):]
    names = [n for n, _ in cls._fields_]
    order = [re.search(r"[\s*]" + n + r"[;,]", body).start() for n in names]    # the declarators
    assert order == sorted(order)
    want = {"bpmx_hrvspec_params": ["win", "hop", "dmin", "dmax", "min_intervals", "min_span", "n_freq", "lf_a", "lf_b",
                                    "hf_a", "hf_b", "reserved", "om0", "dom", "scale"],
            "bpmx_hrvspec_out": ["code", "n_rr", "lf_peak", "hf_peak", "t_mid", "var", "lf", "hf", "q", "record",
                                 "status"]}[struct]
    assert names == want


def test_window_count_at_the_edges():
    L = N.load()
    win, hop = 36240, 9060
    for nd, want in ((-5, 0), (0, 0), (1, 1), (win - 1, 1), (win, 1), (win + 1, 1), (win + hop - 1, 1), (win + hop, 2),
                     (540000, 56), (2 ** 40, (2 ** 40 - win) // hop + 1)):
        assert L.bpmx_hrvspec_windows(nd, win, hop) == want == HS.n_windows(nd, win, hop), nd
    assert L.bpmx_hrvspec_windows(10, 10, 1) == 1 and L.bpmx_hrvspec_windows(10, 1, 1) == 10
    assert L.bpmx_hrvspec_windows(100, 10, 0) == 0 and L.bpmx_hrvspec_windows(100, 0, 1) == 0   # never a division by 0


def _args(q=True, status=True, pk_off=True, final=True, cap=100, **kw):
    one = (ctypes.c_int64 * 2)(0, 0)
    ptr = ctypes.addressof(one)                           # never dereferenced: the arguments are checked first
    p = N.hrvspec_params(dict(HS.geometry(302), **kw))
    k, b, o = N.PackedOut(), N.BeatsOut(), N.HrvspecOut()
    k.cap_peaks, k.pk_off = cap, (ptr if pk_off else None)
    b.final_idx, b.n_final, b.status = (ptr if final else None), ptr, ptr
    for name, _ in N.HrvspecOut._fields_:
        setattr(o, name, ptr)
    if not q:
        o.q = None
    if not status:
        o.status = None
    keep = (one, p, k, b, o)
    return keep, one, [ctypes.byref(p), ctypes.byref(k), ctypes.byref(b), ctypes.byref(o), None]


BAD = [dict(hop=0), dict(dmin=0), dict(dmin=454), dict(min_intervals=2), dict(n_freq=0), dict(n_freq=1025),
       dict(lf_a=-1), dict(lf_a=79), dict(lf_b=257), dict(hf_a=-1), dict(hf_a=257, hf_b=257), dict(hf_b=77),
       dict(hf_b=257), dict(om0=0.0), dict(om0=-1e-3), dict(om0=float("nan")), dict(om0=float("inf")),
       dict(dom=-1e-9), dict(dom=float("nan")), dict(dom=float("inf"))]


def test_argument_errors_name_the_entry_point():
    L = N.load()
    ctx = ctypes.c_void_p(1)                              # never dereferenced either
    err = lambda: L.bpmx_last_error()  # noqa: E731
    keep, fo, a = _args()
    assert L.bpmx_hrvspec_device(None, 1, fo, 1, 302, *a) == N.E_ARG and b"bpmx_hrvspec_device: NULL" in err()
    assert L.bpmx_hrvspec_device(ctx, 1, None, 1, 302, *a) == N.E_ARG and b"bpmx_hrvspec_device: NULL" in err()
    for k in (0, 1, 2, 3):                                # params, tables, beats, out
        b = list(a)
        b[k] = None
        assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *b) == N.E_ARG and b"bpmx_hrvspec_device: NULL" in err(), k
    for F, ds, sr in ((-1, 1, 302), (1, 0, 302), (1, 1, 0)):
        assert L.bpmx_hrvspec_device(ctx, F, fo, ds, sr, *a) == N.E_ARG and b"bad n_files/ds/sr" in err()
    for kw in BAD:
        keep, fo, a = _args(**kw)
        assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG, kw
        assert b"bpmx_hrvspec_device: needs hop >= 1, 1 <= dmin <= dmax, min_intervals >= 3" in err(), kw
        with pytest.raises(ValueError):
            HS.check_geometry(dict(HS.geometry(302), **kw))
    for kw in (dict(dom=0.0), dict(n_freq=1, lf_b=1, hf_a=1, hf_b=1), dict(lf_b=0, hf_a=0), dict(min_span=-3),
               dict(win=0), dict(dmin=453)):                  # the edges that are allowed
        keep, fo, a = _args(pk_off=False, **kw)
        assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"needs pk_off" in err(), kw
    keep, fo, a = _args(win=3600 * 302)                       # an hour per window: too many intervals for the LDS
    assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_LIMIT and b"LDS" in err()
    for cap in (-1, 2 ** 31 - 1):
        keep, fo, a = _args(cap=cap)
        assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"cap_peaks < 2^31" in err()
    keep, fo, a = _args(final=False)
    assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"final_idx, n_final and status" in err()
    keep, fo, a = _args(status=False)
    assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"every pointer of bpmx_hrvspec_out but q" in err()
    keep, fo, a = _args()
    fo[0], fo[1] = 5, 0
    assert L.bpmx_hrvspec_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"non-decreasing" in err()


def test_no_files_is_ok():
    L = N.load()
    keep, fo, a = _args(pk_off=False, final=False, status=False)      # nothing of the arrays is looked at
    assert L.bpmx_hrvspec_device(ctypes.c_void_p(1), 0, fo, 1, 302, *a) == N.OK
    keep, fo, a = _args(hop=0)                                        # the parameters are checked all the same
    assert L.bpmx_hrvspec_device(ctypes.c_void_p(1), 0, fo, 1, 302, *a) == N.E_ARG


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
    exe = str(tmp_path_factory.mktemp("hrvspec_plan") / "hrvspec_core_driver")
    b = subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(HERE, "hrvspec_core_driver.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, "plan", *[":".join(str(v) for v in c) for c in cases]], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in r.stdout.splitlines()]
    return run


def test_structure_sizes_match_the_binding(plan):
    sizes, = plan()
    assert sizes["sizeof_params"] == ctypes.sizeof(N.HrvspecParams)
    assert sizes["sizeof_out"] == ctypes.sizeof(N.HrvspecOut)
    assert sizes["threads"] == 256 and sizes["rec_threads"] == 64 and sizes["record"] == N.HRVSPEC_RECORD
    assert sizes["block"] == sizes["parts"] and sizes["threads"] % sizes["parts"] == 0 and 64 % sizes["parts"] == 0
    assert sizes["max_freq"] == 1024 and sizes["per"] == 32
    # a workgroup's dynamic LDS and its static arrays (q, one sum, count and pick per thread) fit 64 KB
    static = 8 * sizes["max_freq"] + sizes["threads"] * (8 + 4 + sizes["sizeof_pick"])
    assert sizes["lds_max"] + static <= 64 * 1024


def test_lds_limit(plan):
    g = HS.geometry(302)
    sizes, d302, d1000, at, over, tiny, nowin = plan((g["win"], g["dmin"]), (120000, 250), (1535 * 10, 10),
                                                      (1536 * 10, 10), (5, 10), (0, 76))
    assert d302 == dict(status=0, nmax=g["win"] // g["dmin"] + 1, lds=32 * (g["win"] // g["dmin"] + 1))
    assert d302["lds"] < 16 * 1024                                    # the defaults: under 16 KB
    assert d1000["status"] == 0 and d1000["nmax"] == 481
    # the limit is the header's formula, to the byte
    lim = sizes["lds_max"]
    assert at == dict(status=0, nmax=1536, lds=lim) and over["status"] == N.E_LIMIT and over["lds"] == 0
    txt = open(HEADER).read()
    assert "32 * (win / dmin + 1) <= 49152" in txt and lim == 49152
    assert tiny == dict(status=0, nmax=1, lds=32) and nowin["status"] == 0
    assert plan((2 ** 31 - 1, 1))[1]["status"] == N.E_LIMIT            # no overflow on the way to the limit
