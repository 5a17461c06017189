"""bpmx_tempo_device without a GPU: the ABI (exports, structure field order and
sizes against the header text, the option bits, the version), the window count
at its edges, the argument errors, and the plan's limit through the host
driver (tests/tempo_core_driver.cpp in its ``plan`` mode)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import tempo as TP

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bpmx.h")


def test_exports_and_structures():
    assert "bpmx_tempo_device" in N.EXPORTS and "bpmx_tempo_windows" in N.EXPORTS
    L = N.load()
    assert hasattr(L, "bpmx_tempo_device") and hasattr(L, "bpmx_tempo_windows")
    assert ctypes.sizeof(N.TempoParams) == 32 and ctypes.sizeof(N.TempoOut) == 64
    assert N.ABI_VERSION == 4 and L.bpmx_abi_version() == 4      # the entry points are additive
    opts = [getattr(N, k) for k in dir(N) if k.startswith("OPT_")]
    assert len(set(opts)) == len(opts) and all(v & (v - 1) == 0 for v in opts)
    p = N.TempoParams(2416, 604, 76, 453, 0.3, 3, 0)
    assert (p.win, p.hop, p.kmin, p.kmax, p.min_strength, p.start_windows) == (2416, 604, 76, 453, 0.3, 3)


def test_header_and_exports_agree():
    txt = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|const char \*)\s*\*?(bpmx_\w+)\(", txt, re.M))
    assert {"bpmx_tempo_device", "bpmx_tempo_windows"} <= declared
    assert declared == set(N.EXPORTS)
    assert "#define BPMX_ABI_VERSION 4" in txt
    note = txt[:txt.index("#define BPMX_ABI_VERSION")][-400:]
    assert "bpmx_tempo_device" in note and "bpmx_tempo_windows" in note
    bits = [int(v) for v in re.findall(r"\bBPMX_OPT_\w+\s*=\s*(\d+)", txt)]
    assert len(set(bits)) == len(bits) and all(v & (v - 1) == 0 for v in bits)
    assert sorted(bits) == sorted(getattr(N, k) for k in dir(N) if k.startswith("OPT_"))
    # only one form of the kernel exists, so there is no option bit for another
    assert "BPMX_OPT_TEMPO" not in txt and not hasattr(N, "OPT_TEMPO_VALU")


@pytest.mark.parametrize("struct,cls", [("bpmx_tempo_params", N.TempoParams), ("bpmx_tempo_out", N.TempoOut)])
def test_field_order_is_the_bindings(struct, cls):
    txt = open(HEADER).read()
    body = txt[:txt.index("} " + struct + ";")]
    body = body[body.rindex("typedef struct {"):]
    names = [n for n, _ in cls._fields_]
    order = [re.search(r"[\s*]" + n + r"[;,]", body).start() for n in names]    # the declarators
    assert order == sorted(order)


def test_window_count_at_the_edges():
    L = N.load()
    win, hop = 2416, 604
    for nd, want in ((0, 0), (win - 1, 0), (win, 1), (win + 1, 1), (win + hop - 1, 1), (win + hop, 2),
                     (18124, 27), (114050, 185), (2 ** 40, (2 ** 40 - win) // hop + 1)):
        assert L.bpmx_tempo_windows(nd, win, hop) == want == TP.n_windows(nd, win, hop), nd
    assert L.bpmx_tempo_windows(10, 10, 1) == 1 and L.bpmx_tempo_windows(10, 1, 1) == 10
    assert L.bpmx_tempo_windows(-1, 4, 1) == 0
    assert L.bpmx_tempo_windows(100, 10, 0) == 0 and L.bpmx_tempo_windows(100, 0, 1) == 0     # never a division by 0


def _args(win=2416, hop=604, kmin=76, kmax=453, strength=0.3, start=3, env=True, hint=True):
    one = (ctypes.c_int64 * 2)(0, 0)
    ptr = ctypes.addressof(one)                           # never dereferenced: the arguments are checked first
    p, i, o = N.TempoParams(win, hop, kmin, kmax, strength, start, 0), N.Out(), N.TempoOut()
    i.env = ptr if env else None
    for name, _ in N.TempoOut._fields_:
        setattr(o, name, ptr)
    if not hint:
        o.hint = None
    keep = (one, p, i, o)
    return keep, one, [ctypes.byref(p), ctypes.byref(i), ctypes.byref(o), None]


def test_argument_errors_name_the_entry_point():
    L = N.load()
    ctx = ctypes.c_void_p(1)                              # never dereferenced either
    err = lambda: L.bpmx_last_error()  # noqa: E731
    keep, fo, a = _args()
    assert L.bpmx_tempo_device(None, 1, fo, 1, 302, *a) == N.E_ARG and b"bpmx_tempo_device: NULL" in err()
    assert L.bpmx_tempo_device(ctx, 1, None, 1, 302, *a) == N.E_ARG and b"bpmx_tempo_device: NULL" in err()
    for k in (0, 1, 2):                                   # params, in, out
        b = list(a)
        b[k] = None
        assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *b) == N.E_ARG and b"bpmx_tempo_device: NULL" in err(), k
    for F, ds, sr in ((-1, 1, 302), (1, 0, 302), (1, 1, 0)):
        assert L.bpmx_tempo_device(ctx, F, fo, ds, sr, *a) == N.E_ARG and b"bad n_files/ds/sr" in err()
    # hop 0, kmin 1, kmax + 1 >= win, an empty lag range
    for kw in (dict(hop=0), dict(kmin=1), dict(kmax=2415), dict(kmax=2416), dict(kmin=454), dict(win=0)):
        keep, fo, a = _args(**kw)
        assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG, kw
        assert b"bpmx_tempo_device: needs hop >= 1, 2 <= kmin <= kmax and kmax + 1 < win" in err(), kw
    keep, fo, a = _args(win=16000, hop=4000, kmin=500, kmax=3000)          # 2 kHz: too wide for the plan
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 2000, *a) == N.E_LIMIT and b"LDS" in err()
    keep, fo, a = _args(win=352800, hop=88200, kmin=11025, kmax=66150)     # an envelope at 44.1 kHz
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 44100, *a) == N.E_LIMIT and b"bpmx_tempo_device" in err()
    keep, fo, a = _args(strength=float("nan"))
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"min_strength" in err()
    keep, fo, a = _args(start=-1)
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"start_windows" in err()
    keep, fo, a = _args(env=False)
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"bpmx_tempo_device: needs env" in err()
    keep, fo, a = _args(hint=False)
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"every pointer of bpmx_tempo_out" in err()
    keep, fo, a = _args()
    fo[0], fo[1] = 5, 0
    assert L.bpmx_tempo_device(ctx, 1, fo, 1, 302, *a) == N.E_ARG and b"non-decreasing" in err()


def test_no_files_is_ok():
    L = N.load()
    keep, fo, a = _args(env=False, hint=False)            # nothing of the arrays is looked at
    assert L.bpmx_tempo_device(ctypes.c_void_p(1), 0, fo, 1, 302, *a) == N.OK
    keep, fo, a = _args(hop=0)                            # the parameters are checked all the same
    assert L.bpmx_tempo_device(ctypes.c_void_p(1), 0, fo, 1, 302, *a) == N.E_ARG


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
    exe = str(tmp_path_factory.mktemp("tempo_plan") / "tempo_core_driver")
    b = subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(HERE, "tempo_core_driver.cpp")],
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
    assert sizes["sizeof_params"] == ctypes.sizeof(N.TempoParams)
    assert sizes["sizeof_out"] == ctypes.sizeof(N.TempoOut)
    assert sizes["threads"] == 256 == 64 * sizes["waves"] and sizes["rec_threads"] == 64
    # a workgroup's dynamic LDS and its static arrays (scan, sums, one pick per thread) fit a CU's 160 KB
    assert sizes["lds_max"] + sizes["threads"] * sizes["sizeof_best"] + 1024 <= 160 * 1024


def test_plan_geometry_and_limit(plan):
    sizes, d302, d147, d1000, wide, odd = plan(TP.geometry(302), TP.geometry(147), TP.geometry(1000),
                                               TP.geometry(1000, dict(min_bpm=30, max_bpm=300)), (203, 51, 7, 61))
    E_ARG, E_LIMIT = N.E_ARG, N.E_LIMIT
    for p, (win, hop, kmin, kmax) in ((d302, TP.geometry(302)), (d147, TP.geometry(147)), (d1000, TP.geometry(1000)),
                                      (wide, TP.geometry(1000, dict(min_bpm=30, max_bpm=300))), (odd, (203, 51, 7, 61))):
        assert p["status"] == 0
        assert p["nlag"] == kmax - kmin + 3 and p["win4"] == -(-win // 4) * 4 and p["win4"] % sizes["step"] == 0
        assert p["lags"] in (5, 7) and p["lags"] % 2 == 1                 # odd: the lanes' reads miss each other's banks
        assert p["lags"] <= sizes["pad"] - 1
        # the waves' pieces are whole steps and cover the window
        assert p["chunk"] % sizes["step"] == 0 and sizes["waves"] * p["chunk"] >= p["win4"]
        # the last read of the sliding window: sample win4 - 1 of the last lag a lane may hold
        assert p["win4"] - 1 + kmax + 1 + p["lags"] - 1 < p["elen"]
        assert p["pstride"] >= p["nlag"]
        assert p["lds"] == 8 * (p["elen"] + sizes["waves"] * p["pstride"]) <= sizes["lds_max"]
    assert d302["lds"] <= 40 * 1024                                       # four workgroups share a CU at the usual rate
    assert odd["win4"] == 204
    # the limit is the header's formula, to the byte
    lim = sizes["lds_max"]
    fits = lambda win, kmin, kmax: 8 * (-(-win // 4) * 4 + kmax + 8 + 4 * (kmax - kmin + 4)) <= lim  # noqa: E731
    kmin = 100
    kmax = max(k for k in range(kmin, 8000) if fits(8000, kmin, k))
    at, over = plan((8000, 2000, kmin, kmax), (8000, 2000, kmin, kmax + 1))[1:]
    assert at["status"] == 0 and at["lds"] <= lim < at["lds"] + 40 and over["status"] == E_LIMIT and over["lds"] == 0
    txt = open(HEADER).read()
    assert "8 * (win4 + kmax + 8 + 4 * (kmax - kmin + 4)) <= 155648" in txt and lim == 155648
    # the argument checks come first
    for c in ((2416, 0, 76, 453), (2416, 604, 1, 453), (2416, 604, 76, 2415), (2416, 604, 454, 453),
              (2 ** 31 - 1, 1, 2, 2 ** 31 - 2)):
        assert plan(c)[1]["status"] == E_ARG, c
    assert plan((2 ** 31 - 1, 1, 2, 2 ** 31 - 3))[1]["status"] == E_LIMIT     # no overflow on the way to the limit
