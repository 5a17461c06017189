"""The host's kernel selection and launch geometry (csrc/bpmx_plan.h), read
without a GPU: tests/plan_driver.hip is compiled as a host program and prints
detect_plan / ref_env_plan for the cases below.  The expected values are the
switch points and sizes of the run sequencer as it stood before the plans were
split out of it; a change of any of them is a change of behaviour."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

STAGE_FLOOR, STAGE_PEAKS = 2, 4
OPT_ROLLQ_MERGE, OPT_DRAFT_FULL, OPT_ROLLQ_NOPRUNE, OPT_ROLLQ_GLOBAL = 1, 8, 16, 64
OPT_PEAKS_GLOBAL, OPT_REF_SERIAL_MEAN, OPT_REF_NOSPLIT = 256, 1024, 8192
E_LIMIT = -3


def test_option_values_match_the_abi():
    from bpm_analysis_amd import _native as N
    assert (N.STAGE_FLOOR, N.STAGE_PEAKS, N.E_LIMIT) == (STAGE_FLOOR, STAGE_PEAKS, E_LIMIT)
    assert (N.OPT_ROLLQ_MERGE, N.OPT_DRAFT_FULL, N.OPT_ROLLQ_NOPRUNE, N.OPT_ROLLQ_GLOBAL, N.OPT_PEAKS_GLOBAL) == \
        (OPT_ROLLQ_MERGE, OPT_DRAFT_FULL, OPT_ROLLQ_NOPRUNE, OPT_ROLLQ_GLOBAL, OPT_PEAKS_GLOBAL)
    assert (N.OPT_REF_SERIAL_MEAN, N.OPT_REF_NOSPLIT) == (OPT_REF_SERIAL_MEAN, OPT_REF_NOSPLIT)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        # a failed plan's line ends with its message, which has blanks
        return [dict(kv.split("=", 1) for kv in ln.split(" ", 2 if ln.startswith("rc=-") else -1)) for ln in lines]
    return run


def _detect(F, nd, W=3020, options=0, ordered=0, min_periods=3, distance=15, stages=STAGE_FLOOR | STAGE_PEAKS):
    return f"detect:{F}:{nd}:{W}:{options}:{ordered}:{min_periods}:{distance}:{stages}"


def _has(d, **want):
    got = {k: d[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}


def test_lengths_at_the_default_window(driver):
    bench, a, b, c, d, e, f, g = driver(
        _detect(1024, 18124), _detect(4, 18432), _detect(4, 18433), _detect(4, 24576), _detect(4, 24577),
        _detect(2, 65536), _detect(2, 65537), _detect(64, 543600))
    _has(bench, rc=0, floor_wm=1, need_merge=0, long_files=0, fp_long=0, bounds=1, cap=3328, db_gy=5, dp_gy=4,
         g2="8,1024", gf="1,1024")
    assert max(int(bench["wm_lds_p"]), int(bench["wm_lds"])) == 160528
    _has(a, floor_wm=1)
    _has(b, floor_wm=0, wm_chunks=1, wm_c=15360, wm_nch=2, need_merge=1, merge_g=0, union="256,16", lds=39452,
         chunk=1024, nch=19)
    _has(c, long_files=0)
    _has(d, long_files=1)
    _has(e, fp_long=0, gf="1,2")
    _has(f, fp_long=1, gf="257,2")
    _has(g, wm_nch=36, chunk=8192, nch=67, g2="32,64")


def test_window_switches(driver):
    ws = (3841, 3842, 7937, 7938, 16385, 16386, 70000)
    p = dict(zip(ws, driver(*[_detect(1, 200000, W=w) for w in ws])))
    _has(p[3841], union="256,16")
    _has(p[3842], union="256,32")
    _has(p[7937], union="256,32", cap=8192, merge_g=0)
    _has(p[7938], merge_g=1, wm_chunks=1, union="g")
    _has(p[16385], wm_c=2048, wm_chunks=1)
    _has(p[16386], wm_chunks=0)
    _has(p[70000], merge_g=1, chunk=70144, nch=3)


def test_limit(driver):
    (d,) = driver(_detect(1, 3000000, W=2500000))
    assert int(d["rc"]) == E_LIMIT
    assert int(d["lds_g"]) == 167568 and 167568 > 163840
    assert d["err"] == "noise window and recording both longer than 2359296 samples"


def test_options(driver):
    merge, glob, noprune, full, pglob, ordered, badw = driver(
        _detect(4, 18124, options=OPT_ROLLQ_MERGE), _detect(4, 18124, options=OPT_ROLLQ_GLOBAL),
        _detect(4, 18124, options=OPT_ROLLQ_NOPRUNE), _detect(4, 18124, options=OPT_DRAFT_FULL),
        _detect(4, 18124, options=OPT_PEAKS_GLOBAL), _detect(4, 70000, ordered=1), _detect(4, 18124, W=2))
    _has(merge, use_wm=0, need_merge=1, merge_g=0, floor_wm=0)
    _has(glob, merge_g=1, chunk=3072, nch=6)
    _has(noprune, use_wm=1, floor_wm=0, need_merge=0)
    _has(full, bounds=0, floor_wm=1)
    _has(pglob, fp_global=1)
    _has(ordered, fp_global=1, fp_long=0)
    _has(badw, bad_window=1, W=3, cap=320)


def test_reference_envelope(driver):
    a, short, nosplit, serial, w1 = driver("ref:18124:30:0", "ref:4095:30:0", f"ref:18124:30:{OPT_REF_NOSPLIT}",
                                           f"ref:18124:30:{OPT_REF_SERIAL_MEAN}", "ref:18124:1:0")
    _has(a, chain=1, rows=18154, nfc=5, wants_split=1, fwd="0,1024,3072,7168,15360,18154", nkc=4,
         kend="9024,13568,15808,18124")
    _has(short, nkc=0, kend="")
    _has(nosplit, wants_split=0)
    _has(serial, chain=0)
    _has(w1, chain=0)
