"""csrc/bpmx_score_core.h (the scoring stated once for host and device) as
plain C++ on the CPU: tests/score_core_driver.cpp, compiled here with the host
compiler, against ``labels.score`` on the shared cases, integers compared for
equality; 1, 2, 7 and 64 threads as the lanes of a workgroup; the millisecond
conversion of the labels' rounded times.  A second build with the address and
undefined-behaviour sanitizers runs the same inputs; it is a stand-alone host
program, never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import labels as LB
from tests import score_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "score_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-pthread"]
RATES = (3, 16, 147, 302, 1000, 2000, 44100, 48000)


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("score_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "score_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _run(exe, workdir, tag, *extra):
    inp, out = str(workdir / "cases.bin"), str(workdir / f"out_{tag}.bin")
    if not os.path.exists(inp):
        SC.write_cases(inp)
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return SC.read_results(out, len(SC.cases()))


def _equals_labels_py(got):
    for (name, det, _), g, want in zip(SC.cases(), got, SC.expected()):
        SC.assert_same(g, want, name)
        SC.check_identities(g["record"], 0 if det is None else len(det["time"]))


@pytest.mark.parametrize("lanes", [1, 2, 7, 64])
def test_core_equals_labels_py(driver, workdir, lanes):
    """The kernel's partition of the work: threads as the lanes of a workgroup, a barrier as sync()."""
    _equals_labels_py(_run(driver, workdir, f"lanes{lanes}", str(lanes)))


def test_cases_cover_the_branches():
    by = {n: w for (n, _, _), w in zip(SC.cases(), SC.expected())}
    assert [by[n]["status"] for n in ("n0", "no_ref", "no_labels", "no_labels_no_ref", "no_det")] == \
        [LB.SCORE_NONE, LB.SCORE_NONE, LB.SCORE_NO_LABELS, LB.SCORE_NONE, LB.SCORE_OK]
    assert by["no_ref"]["record"][LB.SR_N_OUTSIDE] == 65 and by["n0"]["record"].tolist() == [0] * 20
    for n in ("n63", "n129", "n700", f"n{SC.OVER}"):
        r = by[n]["record"]
        assert min(r[LB.SR_TP], r[LB.SR_SWAP], r[LB.SR_FP], r[LB.SR_FN], r[LB.SR_N_OUTSIDE]) > 0, n
        assert r[LB.SR_N_SPANS] >= 2 and SC.TOL_MS - 10 < r[LB.SR_MAX_ABS] <= SC.TOL_MS, n
    assert by["n700"]["record"][LB.SR_MAX_ABS] == SC.TOL_MS              # a match at the edge of the tolerance
    assert len({int(w["record"][LB.SR_N_SPANS]) for w in SC.expected()}) >= 5
    # every generated reference table carries a row of another type and one without a time
    assert all(LB.marks_from_table(ref)["dropped"] == 2 for n, _, ref in SC.cases() if n[1:].isdigit())


def test_milliseconds_of_rounded_times(driver, workdir):
    """llrint(round(idx / sr, 3) * 1000.0) is the integer n with round(idx / sr, 3) == n / 1000.0."""
    out = str(workdir / "ms.bin")
    r = subprocess.run([driver, "ms", out, *map(str, RATES)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, np.int32).reshape(len(RATES), 4096)
    for k, sr in enumerate(RATES):
        t = np.array([round(i / sr, 3) for i in range(4096)])
        assert (got[k] / 1000.0 == t).all(), sr
        assert got[k].tolist() == LB._ms(t).tolist(), sr


def test_sanitizer_build_runs_clean(workdir):
    exe = str(workdir / "score_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    _equals_labels_py(_run(exe, workdir, "san"))
    _equals_labels_py(_run(exe, workdir, "san5", "5"))
