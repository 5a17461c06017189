"""csrc/bpmx_beats_core.h (the beat stages stated once for host and device) as
plain C++ on the CPU: tests/beats_core_driver.cpp, compiled here with the host
compiler, against ``_host.beats_packed`` (everything equal, the curves bit for
bit: same compiler, same operations) and against the reference's beat goldens
(the bars of test_host_beats.py).  A second build with the address and
undefined-behaviour sanitizers runs the same inputs; it is a stand-alone host
program, never loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import beats_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "beats_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall"]


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("beats_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "beats_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def tables():
    gold = [(n, t) for n, _, t in C.golden_tables()]
    return gold + C.oracle_tables() + C.crafted_tables() + [("long", C.long_table())]


@pytest.fixture(scope="module")
def case_file(workdir, tables):
    path = str(workdir / "cases.bin")
    C.write_cases(path, [t for _, t in tables])
    return path


def _run(exe, case_file, out, tables, *extra, env=None):
    r = subprocess.run([exe, case_file, out, *extra], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return C.read_results(out, [t for _, t in tables])


@pytest.fixture(scope="module")
def results(driver, workdir, case_file, tables):
    return _run(driver, case_file, str(workdir / "out.bin"), tables)


def test_core_equals_host_library(results, tables):
    assert len(results) == len(tables)
    for (name, t), got in zip(tables, results):
        assert C.assert_same(got, t, name, curves="bits")


def test_core_meets_the_reference_goldens(results):
    gold = C.golden_tables()
    assert gold
    for (name, g, _), got in zip(gold, results):
        C.assert_golden(got, g, name)


def test_staged_layout_gives_the_same(driver, workdir, case_file, tables, results):
    """The workspace form the kernel keeps in LDS (idx and env copied in front)."""
    staged = _run(driver, case_file, str(workdir / "out_stage.bin"), tables, "stage")
    for (name, _), a, b in zip(tables, results, staged):
        assert a["status"] == b["status"], name
        for k in ("final_peaks", "bpm_times", "bpm", "pass", "tags"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_cases_cover_the_branches(tables):
    """The inputs reach the error path, both refinement corrections and the
    estimated start BPM."""
    hosts = {n: C.host(t) for n, t in tables if not n.startswith("long")}
    assert any("error" in r for r in hosts.values())
    assert any("error" not in r and r["start_bpm"] not in (80.0, 140.0) for r in hosts.values())
    gap, _ = C.refinement_fires(C.long_table())
    assert gap                                        # so fix_discontinuities returned n_fix > 0
    small = [C.refinement_fires(t) for n, t in tables if n.startswith("n300")]
    assert any(g for g, _ in small) and any(s for _, s in small)


def test_sanitizer_build_runs_clean(workdir, case_file, tables, results):
    exe = str(workdir / "beats_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    for extra in ((), ("stage",)):
        got = _run(exe, case_file, str(workdir / "out_san.bin"), tables, *extra)
        for (name, _), a, b2 in zip(tables, results, got):
            assert a["status"] == b2["status"] and a["final_peaks"].tobytes() == b2["final_peaks"].tobytes(), name
            assert a["bpm"].tobytes() == b2["bpm"].tobytes(), name
