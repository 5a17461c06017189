"""csrc/bpmx_tempo_core.h (the tempogram's decisions, stated once for host and
device) as plain C++ on the CPU: tests/tempo_core_driver.cpp, compiled here
with the host compiler, against ``tempo.tempogram_ints`` on the shared cases at
the bounds of tests/tempo_cases.py; 1, 2, 7 and 64 threads as the lanes of a
workgroup.  A second build with the address and undefined-behaviour sanitizers
runs the same inputs; it is a stand-alone host program, never loaded into
Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tempo_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tempo_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-pthread"]


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("tempo_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "tempo_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _run(exe, workdir, tag, *extra):
    inp, out = str(workdir / "cases.bin"), str(workdir / f"out_{tag}.bin")
    if not os.path.exists(inp):
        TC.write_cases(inp)
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return TC.read_results(out, len(TC.cases()))


def _equals_tempo_py(got):
    for c, g, want in zip(TC.cases(), got, TC.expected()):
        TC.check_inputs(c, want)
        TC.assert_close(g, want, c["name"], exact=c["exact"])
        if c["exact"]:                       # every sum is exact: the same doubles in any order
            assert np.array_equal(g["rho"], want["rho"]) and np.array_equal(g["bpm"], want["bpm"]), c["name"]


@pytest.mark.parametrize("lanes", [1, 2, 7, 64])
def test_core_equals_tempo_py(driver, workdir, lanes):
    """The kernel's partition of the work: threads as the lanes of a workgroup, a barrier as sync()."""
    _equals_tempo_py(_run(driver, workdir, f"lanes{lanes}", str(lanes)))


def test_cases_cover_the_branches():
    by = {c["name"]: (c, w) for c, w in zip(TC.cases(), TC.expected())}
    for g in TC.GOLDENS:                                     # no decision of the goldens is open
        c, w = by["golden_" + g]
        op, flat = TC.open_windows(w)
        assert not op.any() and not flat.any(), g
    c, w = by["golden_vulpine"]
    assert len(w["lag"]) == 185 and w["n_valid"] == 185
    c, w = by["golden_ref_44k_10s_zeros"]                    # an all-zero envelope: max == min in every window
    assert len(w["lag"]) == 2 and w["n_valid"] == 0 and np.isnan(w["hint"]) and np.isnan(w["mean_rho"])
    c, w = by["constant_window"]
    assert w["lag"][0] == 0 and w["lag"][1] != 0 and w["rho"][0] == 0.0 and np.isnan(w["bpm"][0])
    c, w = by["one_nan"]
    bad = [k for k in range(len(w["lag"])) if k * TC.HOP <= TC.WIN + 7 < k * TC.HOP + TC.WIN]
    assert bad and (w["lag"][bad] == 0).all() and w["n_valid"] == len(w["lag"]) - len(bad)
    c, w = by["inf"]
    assert w["lag"][0] == 0 and (w["lag"][6:10] == 0).all() and (w["lag"][[1, 5, 10]] != 0).all()   # +inf at 3, -inf at 217
    c, w = by["no_candidate"]                                # finite and not constant, yet invalid
    assert len(w["lag"]) > 1 and (w["lag"] == 0).all() and np.isfinite(c["env"]).all()
    c, w = by["equal_best"]
    assert w["gap"][0] == 0.0 and w["lag"][0] == TC.TIE[1] and c["exact"]
    e = np.concatenate([c["env"] - c["env"].mean(), np.zeros(c["kmax"] + 1)])
    r = np.array([e[:c["win"]] @ e[k:k + c["win"]] for k in range(c["kmax"] + 2)])
    ties = [k for k in range(c["kmin"], c["kmax"] + 1) if r[k] == r[w["lag"][0]] and r[k] > r[k - 1] and r[k] >= r[k + 1]]
    assert len(ties) >= 2 and min(ties) == w["lag"][0]      # the smallest of the equal candidates
    c, w = by["plateau"]
    assert w["d_hi"][0] == 0.0 and w["lag"][0] == TC.PLATEAU[1] and w["gap"][0] > 0
    assert [len(by[f"nd_{n}"][1]["lag"]) for n in (TC.WIN - 1, TC.WIN, TC.WIN + TC.HOP - 1, TC.WIN + TC.HOP)] == [0, 1, 1, 2]
    c, w = by["all_weak"]
    assert w["n_valid"] == len(w["lag"]) > 3 and w["n_strong"] == 0 and np.isnan(w["hint"]) and np.isnan(w["median_bpm"])
    assert not np.isnan(w["mean_rho"])
    c, w = by["weak_then_strong"]
    assert w["rho"][0] < c["min_strength"] <= w["rho"][1] and w["hint"] == w["bpm"][1]
    c, w = by["hint_from_none"]
    assert w["n_strong"] > 0 and np.isnan(w["hint"])
    assert by["strong_4"][1]["n_strong"] == 4 and by["strong_5"][1]["n_strong"] == 5
    for n in ("strong_4", "strong_5"):
        w = by[n][1]
        assert w["median_bpm"] == np.median(w["bpm"]) and len(set(w["bpm"])) == len(w["bpm"])
    c, w = by["median_of_some"]
    assert 0 < w["n_strong"] <= w["n_valid"] and len(w["lag"]) > 64      # more windows than lanes
    c, w = by["odd_ints"]
    assert c["win"] % 4 and (c["kmax"] - c["kmin"] + 3) % 16 and w["n_valid"] > 0


def test_sanitizer_build_runs_clean(workdir):
    exe = str(workdir / "tempo_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    _equals_tempo_py(_run(exe, workdir, "san"))
    _equals_tempo_py(_run(exe, workdir, "san5", "5"))
