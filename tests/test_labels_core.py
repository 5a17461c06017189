"""csrc/bpmx_labels_core.h (the labeler's output stated once for host and
device) as plain C++ on the CPU: tests/labels_core_driver.cpp, compiled here
with the host compiler, against ``labels.py`` and the fixtures the reference
labeler's own functions made, bit for bit; the decimal rounding against
Python's ``round`` and ``float(f"{x:.3f}")``; the nearest-row rule on exact
ties.  A second build with the address and undefined-behaviour sanitizers runs
the same inputs; it is a stand-alone host program, never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import labels_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "labels_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-pthread"]
RATES = (3, 16, 302, 1000, 2000, 44100)


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("labels_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "labels_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def tie_case():
    """sr = 1000: S2 marks exactly midway between two curve rows, and on rows of equal time."""
    raw = np.array([1000, 1500, 2000, 2500, 3000, 3500, 4000, 4600], np.int64)
    tags = np.array([1, 2, 1, 2, 1, 2, 1, 1], np.int8)
    return dict(raw=raw, tags=tags, gap=np.zeros(8, np.int32), strings=None, fin=raw[tags == 1],
                bt=np.array([1.0, 2.0, 3.0, 3.0]), bv=np.array([60.0, 61.0, 62.0, 63.0]), sr=1000, status=0,
                types=tags.copy())


def crafted_cases():
    rng = np.random.default_rng(11)
    out = [("tie", tie_case())]
    for n in (0, 1, 2, 3, 63, 64, 65, 129, 700):         # sizes around the lanes' pieces of the compactions
        raw = np.cumsum(rng.integers(20, 400, n)).astype(np.int64)
        types = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int8)
        if n >= 10:
            types[rng.random(n) < 0.1] = 0
        fin = raw[types == 1]
        m = max(len(fin) - 1, 0)
        bt = fin[1:].astype(np.float64) / 302 if m else np.zeros(0)
        bv = rng.uniform(50, 180, m)
        if m > 3:
            bv[:2] = np.nan
        tags = np.where(types == 2, 2, np.where(types == 1, 3, 4)).astype(np.int8)
        out.append((f"n{n}", dict(raw=raw, tags=tags, gap=np.zeros(n, np.int32), strings=None, fin=fin, bt=bt, bv=bv,
                                  sr=302, status=0, types=types)))
    c = dict(out[-1][1])
    out.append(("bad_status", dict(c, status=-2)))
    out.append(("nan_curve", dict(c, bv=np.full(len(c["bv"]), np.nan))))
    out.append(("no_s2", dict(c, tags=np.where(c["types"] == 1, 1, 4).astype(np.int8),
                              types=np.where(c["types"] == 1, 1, 0).astype(np.int8))))
    return out


@pytest.fixture(scope="module")
def cases():
    return ([(n, c) for n, _, c in LC.golden_cases() if c is not None] + [(n, c) for n, _, c in LC.random_cases()] +
            crafted_cases())


def _run(exe, workdir, cases, tag, gap, *extra):
    inp, out = str(workdir / f"cases_{gap}.bin"), str(workdir / f"out_{tag}_{gap}.bin")
    if not os.path.exists(inp):
        LC.write_cases(inp, [c for _, c in cases], gap)
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return LC.read_results(out, len(cases))


@pytest.fixture(scope="module")
def results(driver, workdir, cases):
    return {gap: _run(driver, workdir, cases, "plain", gap) for gap in LC.GAPS}


def test_core_equals_labels_py_bit_for_bit(results, cases):
    seen = set()
    for gap in LC.GAPS:
        for (name, c), got in zip(cases, results[gap]):
            want = LC.host(c, gap)
            LC.assert_same(LC.labels_of(got, gap), want, (name, gap))
            seen.add(got["status"])
            if want is not None:
                assert got["record"][N.LR_N_S1] == want["summary"]["n_s1"], name
                assert got["record"][N.LR_N_S2] == want["summary"]["n_s2"], name
    assert seen == {N.LABELS_OK, N.LABELS_NONE}


def test_core_meets_the_labeler_fixtures(results, cases):
    """The tags + gap rule gives the rule on the strings, and every number is the labeler's."""
    fx = {n: f for n, f, _ in LC.golden_cases()}
    fx.update({n: f for n, f, _ in LC.random_cases()})
    n_ok = n_groups = 0
    for gap in LC.GAPS:
        for (name, c), got in zip(cases, results[gap]):
            if name not in fx:
                continue
            want = LC.expected(fx[name], gap)
            if name.startswith("random") and LC.host(c, gap) is None:
                want = None                           # fewer than two S1 marks: the stage makes no labels
            LC.assert_same(LC.labels_of(got, gap), want, (name, gap))
            n_ok += want is not None
            n_groups = max(n_groups, 0 if want is None else len(want["groups"]["id"]))
    assert n_ok >= 3 * (26 + 40) and n_groups >= 5
    assert int(fx["env_plateaus"]["s1_string_not_final"]) == 19 and int(fx["ref_44k_40s_clicks"]["s1_string_not_final"]) == 3


def test_rounding_is_pythons(driver, workdir):
    out = str(workdir / "round.bin")
    r = subprocess.run([driver, "round", out, *map(str, RATES)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, np.float64).reshape(len(RATES), 4096)
    differs = 0
    for k, sr in enumerate(RATES):
        for i in range(4096):
            x = i / sr
            assert got[k, i] == round(x, 3) == float(f"{x:.3f}"), (sr, i)
            differs += got[k, i] != np.round(x, 3)
    assert got[RATES.index(2000), 1] == 0.001 and np.round(1 / 2000, 3) == 0.0
    assert differs > 0                                # numpy's multiply-rint-divide is another function


def test_nearest_row_ties_take_the_first(results, cases):
    i = [n for n, _ in cases].index("tie")
    got = results[5.0][i]
    c = cases[i][1]
    T, B = LB.csv_rows(c["bt"], c["bv"])
    assert np.abs(T - 1.5)[0] == np.abs(T - 1.5)[1] and np.abs(T - 1.5).argmin() == 0
    # 1.5 -> row 0 (60), 2.5 -> row 1 (61), 3.0 .. 4.6 -> the first of the two rows at 3.0 (62)
    assert got["lb_time"].tolist() == [1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.6]
    assert got["lb_bpm"].tolist() == [60.0, 60.0, 61.0, 61.0, 62.0, 62.0, 62.0, 62.0]


def test_cases_cover_the_branches(results, cases):
    by = {n: r for (n, _), r in zip(cases, results[1])}
    assert [by[f"n{n}"]["status"] for n in (0, 1, 2, 3)] == [N.LABELS_NONE] * 3 + [N.LABELS_OK]
    assert by["bad_status"]["status"] == by["nan_curve"]["status"] == N.LABELS_NONE
    assert len(by["no_s2"]["lb_pos"]) > 0 and len(by["no_s2"]["pr_dt"]) == 0 and len(by["no_s2"]["gr_id"]) == 0
    assert np.isnan(by["no_s2"]["record"][:2]).all() and by["no_s2"]["record"][N.LR_N_S2] == 0
    assert len(by["random5"]["lb_pos"]) == 0 or by["random5"]["status"] == N.LABELS_NONE   # no S1 at all
    assert len(by["n700"]["lb_pos"]) > 600 and len(by["n700"]["pr_dt"]) > 250
    ids = [r["gr_id"] for r in results[1]]
    assert any(len(g) >= 2 and (np.diff(g) > 1).any() for g in ids)         # a skipped group keeps its number
    assert any(len(g) >= 5 for g in ids)
    assert any((c["gap"] != 0).any() for _, c in cases)


def _same_raw(cases, a, b):
    for (name, _), x, y in zip(cases, a, b):
        assert x["status"] == y["status"] and x["record"].tobytes() == y["record"].tobytes(), name
        for k in LC.DEV_KEYS_I + LC.DEV_KEYS_F:
            assert x[k].tobytes() == y[k].tobytes(), (name, k)


@pytest.mark.parametrize("lanes", [2, 7, 64])
def test_many_lanes_give_the_same(driver, workdir, cases, results, lanes):
    """The kernel's partition of the work: threads as the lanes of a workgroup, a barrier as sync()."""
    _same_raw(cases, results[1], _run(driver, workdir, cases, f"lanes{lanes}", 1, str(lanes)))


def test_sanitizer_build_runs_clean(workdir, cases, results):
    exe = str(workdir / "labels_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtime inside the program where the compiler has it as an archive, else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = subprocess.run([_cxx(), *BASE, *san, *link, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    _same_raw(cases, results[1], _run(exe, workdir, cases, "san", 1))
    _same_raw(cases, results[1], _run(exe, workdir, cases, "san5", 1, "5"))
