"""csrc/bpmx_hrvspec_core.h (the HRV spectrum's per-window arithmetic, stated
once for host and device) as plain C++ on the CPU: tests/hrvspec_core_driver.cpp,
compiled here with the host compiler, against ``hrv_spectrum.spectrum_ints`` on
the shared cases at the derived bound of tests/hrvspec_cases.py; 1, 2, 7 and 64
threads as the lanes of a workgroup, in both forms (the rotation along the grid
and one sincos per term).  A second build with the address and
undefined-behaviour sanitizers runs the same inputs; it is a stand-alone host
program, never loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import hrvspec_cases as HC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hrvspec_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-pthread"]


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("hrvspec_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "hrvspec_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _run(exe, workdir, tag, *extra):
    inp, out = str(workdir / "cases.bin"), str(workdir / f"out_{tag}.bin")
    if not os.path.exists(inp):
        HC.write_cases(inp)
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return HC.read_results(out)


def _equals_oracle(got):
    used = 0.0
    for c, g, want in zip(HC.cases(), got, HC.expected()):
        assert HC.open_peaks(want) == [], c["name"]
        used = max(used, HC.assert_close(g, want, c["name"]))
    print(f"largest share of the bound on q used: {used:.2e}")
    assert used < 1.0


@pytest.mark.parametrize("form", ["rotate", "direct"])
@pytest.mark.parametrize("lanes", [1, 2, 7, 64])
def test_core_equals_spectrum_ints(driver, workdir, lanes, form):
    """Threads as the lanes of a workgroup, a barrier as sync()."""
    _equals_oracle(_run(driver, workdir, f"lanes{lanes}_{form}", str(lanes), *(["direct"] if form == "direct" else [])))


def test_sanitizer_build_runs_clean(workdir):
    exe = str(workdir / "hrvspec_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    _equals_oracle(_run(exe, workdir, "san"))
    _equals_oracle(_run(exe, workdir, "san5", "5"))
    _equals_oracle(_run(exe, workdir, "san3d", "3", "direct"))
