"""csrc/bpmx_rect_core.h (the rectified-mode envelope's arithmetic, stated once
for the kernels and the host) as plain C++ on the CPU: tests/rect_core_driver.cpp
against the pandas recipe, bit for bit.  For integer PCM of one or two channels
the exact-sum formula and the RollMean recursion must both give the pandas
bits.  A second build with the address and undefined-behaviour sanitizers runs
the same inputs as a stand-alone program; nothing here is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rect_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rect_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall"]
WINDOWS = (1, 2, 3, 30, 31, 32, 1500)          # 1500: larger than every length below


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


def _lengths(w):
    return sorted({n for n in (1, 2, w - 1, w, w + 1, 1000) if 1 <= n <= 1000})


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20240611)
    out = []
    for name in C.DTYPES:
        for ch in (1, 2, 3):
            for w in WINDOWS:
                for n in _lengths(w):
                    out.append((f"{name}-c{ch}-w{w}-n{n}", C.make(rng, name, n, ch), w))
    for name in C.INT_NAMES:
        for ch in (1, 2):
            for kind in ("allmin", "zeros"):
                for w in (1, 2, 30, 31):
                    out.append((f"{name}-c{ch}-w{w}-{kind}", C.make_int(rng, name, 100, ch, kind), w))
    return out


@pytest.fixture(scope="module")
def expected(cases):
    return [C.recipe(pcm, w) for _, pcm, w in cases]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("rect_core")


@pytest.fixture(scope="module")
def case_file(workdir, cases):
    path = str(workdir / "cases.bin")
    C.write_cases(path, [(pcm, w) for _, pcm, w in cases])
    return path


def _run(exe, case_file, out, cases):
    r = subprocess.run([exe, case_file, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return C.read_results(out, [(pcm, w) for _, pcm, w in cases])


@pytest.fixture(scope="module")
def results(workdir, case_file, cases):
    exe = str(workdir / "rect_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return _run(exe, case_file, str(workdir / "out.bin"), cases)


def test_recursion_equals_pandas(results, cases, expected):
    assert len(results) == len(cases)
    for (name, _, _), (gen, _), want in zip(cases, results, expected):
        assert C.same_bits(gen, want), name


def test_exact_sums_equal_pandas_and_the_recursion(results, cases, expected):
    seen = 0
    for (name, pcm, _), (gen, ex), want in zip(cases, results, expected):
        eligible = pcm.dtype.kind in "iu" and (pcm.ndim == 1 or pcm.shape[1] <= 2)
        assert (ex is not None) == eligible, name
        if eligible:
            seen += 1
            assert C.same_bits(ex, want), name
            assert ex.tobytes() == gen.tobytes(), name
    assert seen >= 3 * 2 * len(WINDOWS)


def test_cases_cover_the_special_values(cases, expected):
    """Negative rectified samples, NaN outputs, inf and -0.0 inputs all occur."""
    assert any(pcm.dtype == np.int16 and pcm.ndim == 1 and (np.abs(pcm) < 0).any() for _, pcm, _ in cases)
    assert any(np.isnan(e).any() for e in expected) and any((e < 0).any() for e in expected)
    fl = [pcm for _, pcm, _ in cases if pcm.dtype.kind == "f"]
    assert any(np.isinf(p).any() for p in fl) and any((np.signbit(p) & (p == 0)).any() for p in fl)
    tiny = np.finfo(np.float32).tiny
    assert any(((np.abs(p) < tiny) & (p != 0)).any() for p in fl if p.dtype == np.float32)


def test_sanitizer_build_runs_clean(workdir, case_file, cases, results):
    exe = str(workdir / "rect_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    got = _run(exe, case_file, str(workdir / "out_san.bin"), cases)
    for (name, _, _), (g0, e0), (g1, e1) in zip(cases, results, got):
        assert g0.tobytes() == g1.tobytes(), name
        assert (e0 is None) == (e1 is None) and (e0 is None or e0.tobytes() == e1.tobytes()), name
