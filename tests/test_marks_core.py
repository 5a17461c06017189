"""csrc/bpmx_marks_core.h (a person's marks as rows, beats and curve, stated
once for host and device) as plain C++ on the CPU: tests/marks_core_driver.cpp,
compiled here with the host compiler, against ``labels.rows_from_marks`` and
``beats.bpm_series`` on the shared cases, integers compared for equality and
doubles as bit patterns; 1, 2, 7 and 64 threads as the lanes of a workgroup.  A
second build with the address and undefined-behaviour sanitizers runs the same
inputs; it is a stand-alone host program, never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import labels as LB
from tests import marks_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "marks_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-pthread"]


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("marks_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "marks_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _run(exe, workdir, tag, *extra):
    inp, out = str(workdir / "cases.bin"), str(workdir / f"out_{tag}.bin")
    if not os.path.exists(inp):
        MC.write_cases(inp)
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return MC.read_results(out, len(MC.cases()))


def _equals_labels_py(got):
    for c, g, want in zip(MC.cases(), got, MC.expected()):
        MC.assert_same(g, want, c["name"])
        MC.check_identity(g["record"], len(c["ms"]))
        n = len(g["idx"])
        assert not g["gap"].any() and np.isnan(g["env"]).all() and np.isnan(g["floor"]).all(), c["name"]
        assert np.isnan(g["pass"]).all() and len(g["env"]) == n, c["name"]
        assert (np.diff(g["idx"].astype(np.int64)) > 0).all(), c["name"]     # what bpmx_labels_device requires


@pytest.mark.parametrize("lanes", [1, 2, 7, 64])
def test_core_equals_labels_py(driver, workdir, lanes):
    """The kernel's partition of the work: threads as the lanes of a workgroup, a barrier as sync()."""
    _equals_labels_py(_run(driver, workdir, f"lanes{lanes}", str(lanes)))


def test_cases_cover_the_branches():
    by = {c["name"]: w for c, w in zip(MC.cases(), MC.expected())}
    rec = lambda n: by[n]["record"].tolist()[:6]  # noqa: E731
    assert rec("n0") == [0] * 6 and rec("one_s1") == [1, 1, 0, 0, 0, 0] and rec("one_s2") == [1, 0, 1, 0, 0, 0]
    assert rec("adjacent") == [2, 2, 0, 0, 0, 0] and by["adjacent"]["status"] == LB.MARKS_OK
    assert by["adjacent"]["idx"].tolist() == [500, 501] and len(by["adjacent"]["bpm"]) == 1
    for n in ("same_sample", "same_sample_s2_first"):                        # S1 wins whichever comes first
        assert rec(n) == [1, 1, 0, 1, 0, 0] and by[n]["status"] == LB.MARKS_FEW
    assert rec("only_s2") == [5, 0, 5, 0, 0, 0] and by["only_s2"]["status"] == LB.MARKS_FEW
    assert rec("negative") == [4, 2, 2, 0, 2, 0]
    assert rec("int32_max")[LB.MK_N_DROPPED] == 3 and by["int32_max"]["idx"][-1] > 2 ** 31 - 64
    assert rec("nd_edge") == [4, 3, 1, 0, 2, 0] and by["nd_edge"]["idx"][-1] == MC.ND_EDGE - 1
    assert rec("nd_zero") == [0, 0, 0, 0, 4, 0]
    assert rec("other_types") == [3, 2, 1, 0, 0, 4]
    low = [n for n in by if n.endswith("_sr3") and n != "n3_sr3"]
    assert len(low) >= 3
    for n in low:                                                             # three samples a second: marks share one
        r = by[n]["record"]
        assert r[LB.MK_N_MERGED] > 0 and r[LB.MK_N_DROPPED] == 1, n
    r = by["n700_sr1000"]["record"]
    assert min(r[:6]) > 0                                                     # every count is exercised at once
    assert {c["sr"] for c in MC.cases()} == set(MC.RATES)
    for n in (MC.LIMIT, MC.LIMIT + 8):
        assert rec(f"s1_{n}")[:2] == [n, n]
    # beat times 2500, 2499 and 2501 ms apart around a 5 s window: 2500 is outside (open left), inside (closed right)
    b = by["window_edges"]
    t = b["bpm_t"]
    assert np.rint(np.diff(t) * 1000).tolist() == [2500, 2499, 2501, 1000, 2500]
    inst = 60.0 / np.diff(np.concatenate([[0.0], t]))
    assert b["bpm"][1] == (inst[1] + inst[2]) / 2 or b["bpm"][1] == np.mean(inst[1:3])      # 1.0 s is outside, 5.999 s inside
    assert b["bpm"][0] == np.mean(inst[0:2])                                  # 3.5 s = 1.0 + 2.5: inside (closed right)


def test_sanitizer_build_runs_clean(workdir):
    exe = str(workdir / "marks_core_driver_san")
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
