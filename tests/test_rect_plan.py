"""The rectified-mode envelope's route and launch geometry (rect_plan in
csrc/bpmx_plan.h), read without a GPU: tests/rect_plan_driver.hip is compiled as
a host program.  Both sides of every switch the plan has: integer or general
route (dtype, channels, option, the window at the exactness bound and one
above), the LDS or the global-prefix variant at its window limit and one above,
and the chunk counts around a chunk boundary."""
import os
import shutil
import subprocess

import pytest

from tests import rect_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
U8, I16, I32, F32, F64 = 0, 1, 2, 3, 4
OPT_RECT_SEQ = 65536


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("rect_plan") / "rect_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "rect_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        args = [f"rect:{dt}:{ch}:{w}:{opt}:{F}:{n}" for dt, ch, w, opt, F, n in cases]
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return [dict(kv.split("=", 1) for kv in ln.split(" ")) for ln in lines]
    return run


def _has(d, **want):
    assert {k: d[k] for k in want} == {k: str(v) for k, v in want.items()}


def test_constants(plan):
    d, = plan((I16, 1, 30, 0, 1, 1000))
    k = C.plan_constants()
    _has(d, chunk=k["RECT_CHUNK"], lds_n=k["RECT_LDS_N"], threads=k["RECT_T"], w_exact_max=2 ** 21 - 1)
    # w * 2^32 < 2^53 at the bound and not above it
    assert (2 ** 21 - 1) * 2 ** 32 < 2 ** 53 <= 2 ** 21 * 2 ** 32
    # the LDS prefix and the scan's four wave totals fit a workgroup's 64 KB
    assert k["RECT_LDS_N"] * 8 + 64 <= 65536 and k["RECT_LDS_N"] % k["RECT_T"] == 0
    assert 2 * k["RECT_CHUNK"] <= k["RECT_LDS_N"]


def test_integer_or_general_by_dtype_channels_and_option(plan):
    cases = [(dt, ch, 30, 0, 4, 5000) for dt in (U8, I16, I32, F32, F64) for ch in (1, 2, 3)]
    for (dt, ch, *_), d in zip(cases, plan(*cases)):
        integer = dt <= I32 and ch <= 2
        _has(d, integer=int(integer), route="int_lds" if integer else "general")
    seq, = plan((I16, 1, 30, OPT_RECT_SEQ, 4, 5000))
    _has(seq, integer=0, route="general", rows_bytes=5056 * 4 * 8, g_pick="79,1", g_seq=1)
    many, = plan((F64, 1, 30, 0, 65, 64))
    _has(many, g_pick="1,2", g_seq=2, rows_bytes=64 * 65 * 8)


def test_window_at_the_exactness_bound(plan):
    at, above = plan((I32, 2, 2 ** 21 - 1, 0, 1, 10 ** 6), (I32, 2, 2 ** 21, 0, 1, 10 ** 6))
    _has(at, integer=1, route="int_global")
    _has(above, integer=0, route="general")


def test_lds_variant_at_its_window_limit(plan):
    k = C.plan_constants()
    T, L = k["RECT_CHUNK"], k["RECT_LDS_N"]
    at, above = plan((I16, 1, L - T, 0, 2, 100000), (I16, 1, L - T + 1, 0, 2, 100000))
    _has(at, route="int_lds", lds=L * 4, csum_bytes=0)
    _has(above, route="int_global", lds=2 * T * 4, csum_bytes=2 * 49 * 8, nch=49)
    # int32 PCM keeps 64-bit local prefixes
    at32, above32 = plan((I32, 2, L - T, 0, 2, 100000), (I32, 1, L - T + 1, 0, 2, 100000))
    _has(at32, route="int_lds", lds=L * 8)
    _has(above32, route="int_global", lds=2 * T * 8)
    # a short batch asks for no more LDS than its prefix needs
    short, = plan((I16, 1, 30, 0, 2, 100))
    _has(short, route="int_lds", lds=101 * 4)
    usual, = plan((I16, 1, 30, 0, 1024, 18124))
    _has(usual, route="int_lds", lds=(T + 30) * 4, grid="9,1024", nch=9)
    assert 4410 + T <= L and 4800 + T <= L < 38400 + T       # 44.1 and 48 kHz in LDS, 384 kHz beyond


def test_chunk_counts_around_a_boundary(plan):
    T = C.plan_constants()["RECT_CHUNK"]
    for w in (30, 38400):
        a, b, c, one = plan((I16, 1, w, 0, 3, 2 * T - 1), (I16, 1, w, 0, 3, 2 * T), (I16, 1, w, 0, 3, 2 * T + 1),
                            (I16, 1, w, 0, 3, 1))
        _has(a, nch=2, grid="2,3")
        _has(b, nch=2, grid="2,3")
        _has(c, nch=3, grid="3,3")
        _has(one, nch=1, grid="1,3")
    g, = plan((I16, 1, 38400, 0, 3, 2 * T + 1))
    _has(g, csum_bytes=3 * 3 * 8)
