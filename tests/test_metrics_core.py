"""csrc/bpmx_metrics_core.h (the final metrics stated once for host and device)
as plain C++ on the CPU: tests/metrics_core_driver.cpp, compiled here with the
host compiler, against ``beats.final_metrics`` on the same beats and curve
(every position and count equal, every double bit for bit: the same IEEE
operations in the same order) and against the reference's recorded metrics in
the beat goldens.  A second build with the address and undefined-behaviour
sanitizers runs the same inputs; it is a stand-alone host program, never
loaded into Python."""
import itertools
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import metrics as MH
from tests import beats_cases as C
from tests import metrics_cases as M
from tests import test_beats as TB

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "metrics_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall"]


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("metrics_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "metrics_core_driver")
    b = subprocess.run([_cxx(), *BASE, "-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def golden():
    """[(name, golden, case)] of the beat goldens that carry metrics."""
    out = [(n, g, M.case(np.asarray(g["final_peaks"]), sr=t["sr"], params=t["params"]))
           for n, g, t in C.golden_tables() if "metrics" in g]
    assert len(out) == 26
    return out


@pytest.fixture(scope="module")
def cases(golden):
    return [(n, c) for n, _, c in golden] + M.crafted_cases() + M.tie_cases()


def _run(exe, workdir, cases, tag, *extra):
    inp, out = str(workdir / "cases.bin"), str(workdir / f"out_{tag}.bin")
    if not os.path.exists(inp):
        M.write_cases(inp, [c for _, c in cases])
    r = subprocess.run([exe, inp, out, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return M.read_results(out, len(cases))


@pytest.fixture(scope="module")
def results(driver, workdir, cases):
    return _run(driver, workdir, cases, "plain")


def test_core_equals_final_metrics_bit_for_bit(results, cases):
    assert len(results) == len(cases)
    for (name, c), got in zip(cases, results):
        assert M.check(got, c, name, bits=True)


def test_core_meets_the_reference_goldens(results, golden):
    """The goldens' own hrv_* arrays and metrics JSON (the reference's output)
    against the dict the host assembles from the core's results."""
    seen = {}
    for (name, g, c), got in zip(golden, results):
        assert got["status"] in (N.METRICS_OK, N.METRICS_TIE), name
        with M.epoch(0):
            m = MH.assemble(c["bt"], c["bv"], got["record"], got["hrv"], got["inc"], got["dec"])
        assert np.array_equal(m["smoothed_bpm"].index.asi8, g["bpm_ns"]), name
        for col in M.HRV_COLS:
            h = m["windowed_hrv_df"]
            TB._close(h[col].to_numpy(float) if len(h) else np.zeros(0), g["hrv_" + col], f"{name} hrv {col}")
        ref = json.loads(str(g["metrics"]))
        for k in ("major_inclines", "major_declines"):
            assert len(m[k]) == len(ref[k]), (name, k)
            for i, (o, r) in enumerate(zip(m[k], ref[k])):
                TB._cmp_obj(o, r, f"{name} {k}[{i}]")
        for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
            TB._cmp_obj(m[k], ref[k], f"{name} {k}")
        assert list(m["hrv_summary"]) == list(ref["hrv_summary"]), name
        for k, v in ref["hrv_summary"].items():
            TB._close(m["hrv_summary"][k], v, f"{name} hrv_summary {k}")
        seen[name] = m
    v = seen["vulpine"]
    assert len(v["major_inclines"]) == 9 and len(v["major_declines"]) == 4
    durs = [float(mm[k]["duration_sec"]) for mm in seen.values()
            for k in ("peak_recovery_stats", "peak_exertion_stats") if mm[k]]
    assert 20.355555999999993 in durs        # differences of total_seconds(), not seconds of the difference
    assert len(seen["env_random_rough"]["major_declines"]) == 1
    n60 = seen["nat_44k_60s_mono"]
    assert n60["peak_recovery_stats"] is not None and n60["hrr_stats"] is None
    full = [n for n, mm in seen.items() if mm["hrr_stats"] and mm["peak_recovery_stats"] and mm["peak_exertion_stats"]]
    assert len(full) >= 2, full


def test_assembled_dict_is_final_metrics(results, cases):
    """metrics.assemble gives the dict beats.final_metrics gives: the same
    Series on the same index, the same table, the same run and stats dicts."""
    n = 0
    for (name, c), got in zip(cases, results):
        want, ref = M.reference(c)
        if want is None or c["custom"] or got["status"] != N.METRICS_OK:
            continue
        with M.epoch(c["epoch_s"]):
            m = MH.assemble(c["bt"], c["bv"], got["record"], got["hrv"], got["inc"], got["dec"])
        assert list(m) == list(ref), name
        pd.testing.assert_series_equal(m["smoothed_bpm"], ref["smoothed_bpm"], check_exact=True, check_freq=False)
        assert np.array_equal(m["bpm_times"], ref["bpm_times"])
        a, b = m["windowed_hrv_df"], ref["windowed_hrv_df"]
        assert list(a.columns) == list(b.columns) and len(a) == len(b), name
        if len(a):
            pd.testing.assert_frame_equal(a, b.astype(np.float64), check_exact=True)
        for k in ("major_inclines", "major_declines"):
            assert len(m[k]) == len(ref[k]), (name, k)
            for x, y in zip(m[k], ref[k]):
                assert list(x) == list(y) and all(x[q] == y[q] for q in y), (name, k)
        for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats", "hrv_summary"):
            x, y = m[k], ref[k]
            assert (x is None) == (y is None), (name, k)
            assert y is None or (list(x) == list(y) and all(x[q] == y[q] for q in y)), (name, k)
        n += 1
    assert n > 40


def test_staged_layout_gives_the_same(driver, workdir, cases, results):
    """The workspace form the kernel keeps in LDS (curve and beats copied in front)."""
    staged = _run(driver, workdir, cases, "stage", "stage")
    for (name, _), a, b in zip(cases, results, staged):
        assert a["status"] == b["status"], name
        assert a["record"].tobytes() == b["record"].tobytes(), name
        for k in ("hrv", "inc", "dec"):
            for q in a[k]:
                assert a[k][q].tobytes() == b[k][q].tobytes(), (name, k, q)


def _filter_outcomes(v, dist, sign):
    """Every outcome of scipy's distance filter over the visiting orders of
    equal heights (None: too many orders to enumerate)."""
    from scipy.signal import find_peaks
    cand = find_peaks(sign * v)[0]
    pr = (sign * v)[cand]
    blocks = [np.flatnonzero(pr == h) for h in sorted(set(pr.tolist()))]
    if np.prod([float(math.factorial(len(b))) for b in blocks]) > 5000:
        return None
    outcomes = set()
    for perms in itertools.product(*[itertools.permutations(b) for b in blocks]):
        order = [j for pp in perms for j in pp]                      # ascending priority
        keep = np.ones(cand.size, dtype=bool)
        for j in reversed(order):
            if keep[j]:
                near = np.abs(cand - cand[j]) < dist
                near[j] = False
                keep[near] = False
        outcomes.add(tuple(cand[keep].tolist()))
    return outcomes


def test_tie_bit_is_exact(results, cases):
    """BPMX_METRICS_TIE is set iff some visiting order of the equal heights
    changes the distance filter's outcome, for the maxima or the minima;
    where it is unset the runs are scipy's (checked bit for bit above)."""
    ties = [(c, got) for (name, c), got in zip(cases, results) if name.startswith("tie")]
    assert len(ties) >= 190
    flagged = checked = 0
    for c, got in ties:
        assert got["status"] in (N.METRICS_OK, N.METRICS_TIE)
        outs = [_filter_outcomes(c["bv"], 5, sg) for sg in (1.0, -1.0)]
        if any(o is None for o in outs):
            continue
        checked += 1
        flagged += got["status"] == N.METRICS_TIE
        assert (got["status"] == N.METRICS_TIE) == any(len(o) > 1 for o in outs), c["bv"].tolist()
        if got["status"] == N.METRICS_OK:
            want, _ = M.reference(c)
            assert M.assert_same(got, want, "tie runs", bits=True, runs=True)
    assert checked >= 150 and 0.1 * checked <= flagged <= 0.9 * checked, (flagged, checked)


def test_cases_cover_the_branches(results, cases):
    """Every status value, an empty and a non-empty result of each kind, both
    sort directions with at least two runs, every branch of the pairwise sum."""
    by = {n: r for (n, _), r in zip(cases, results)}
    sts = {r["status"] for r in results}
    assert {N.METRICS_OK, N.METRICS_TIE, N.METRICS_E_DISTANCE, N.METRICS_NONE} <= sts
    assert [len(by[f"beats{n}"]["hrv"]["time"]) for n in (39, 40, 41, 45, 46)] == [0, 0, 1, 1, 2]
    assert len(by["win64"]["hrv"]["time"]) == 64 and len(by["win65"]["hrv"]["time"]) == 65
    assert all(by[f"n{n}"]["status"] == N.METRICS_NONE for n in (0, 1)) and by["n2"]["status"] == N.METRICS_OK
    assert by["bad_status"]["status"] == N.METRICS_NONE
    for w in (7, 8, 9, 128, 129, 130):
        for step in (1, 5):
            assert len(by[f"w{w}_s{step}"]["hrv"]["time"]) >= 1
    rec = lambda n, i: by[n]["record"][i]  # noqa: E731
    assert np.isnan(rec("dur_under20", N.MR_EXERTION)) and np.isnan(rec("dur_under20", N.MR_RECOVERY))
    assert not np.isnan(rec("dur_over20", N.MR_EXERTION)) or not np.isnan(rec("dur_over20", N.MR_RECOVERY))
    assert np.isnan(rec("hrr_under60", N.MR_HRR_PEAK)) and not np.isnan(rec("hrr_exact60", N.MR_HRR_PEAK))
    assert np.isnan(rec("max_is_last", N.MR_HRR_PEAK)) and np.isnan(rec("max_is_last", N.MR_RECOVERY))
    c = dict(cases)["two_equal_maxima"]
    top = np.flatnonzero(c["bv"] == c["bv"].max())
    assert len(top) >= 2 and rec("two_equal_maxima", N.MR_HRR_PEAK) == top[0]
    const = by["constant_rr"]
    assert rec("constant_rr", N.MR_MIN_BPM) == rec("constant_rr", N.MR_MAX_BPM)
    assert len(const["inc"]["a"]) == 0 and len(const["dec"]["a"]) == 0
    assert by["slow_step_over_5s"]["status"] == N.METRICS_E_DISTANCE
    for off in (3600, -18000):
        assert not np.isnan(rec(f"epoch{off}", N.MR_HRR_PEAK))
    assert any(len(r["inc"]["a"]) >= 2 for r in results) and any(len(r["dec"]["a"]) >= 2 for r in results)
    assert any(len(r["inc"]["a"]) == 0 and r["status"] == 0 for r in results)
    for k in (N.MR_HRR_PEAK, N.MR_RECOVERY, N.MR_EXERTION, N.MR_AVG_RMSSDC):
        vals = [np.isnan(r["record"][k]) for r in results if r["status"] >= 0]
        assert any(vals) and not all(vals), k


def test_sanitizer_build_runs_clean(workdir, cases, results):
    exe = str(workdir / "metrics_core_driver_san")
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
        got = _run(exe, workdir, cases, "san" + "".join(extra), *extra)
        for (name, _), a, b2 in zip(cases, results, got):
            assert a["status"] == b2["status"] and a["record"].tobytes() == b2["record"].tobytes(), name
            for k in ("hrv", "inc", "dec"):
                for q in a[k]:
                    assert a[k][q].tobytes() == b2[k][q].tobytes(), (name, k, q)
