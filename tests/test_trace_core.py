"""The decision trace of csrc/bpmx_beats_core.h (``beats_trace``) as plain C++ on
the CPU (tests/trace_core_driver.cpp) and ``bpm_analysis_amd.explain`` on top
of it: the reference's own debug strings, belief curve and deviation series
(tests/golden/beats), the Python route (``beats.analyze_recording``) on
crafted tables, the report files, and the C ABI of the new entry points.
Everything is compared for equality.  A second build with the address and
undefined-behaviour sanitizers runs the same inputs as a stand-alone host
program, never loaded into Python."""
import ctypes
import os
import re

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from bpm_analysis_amd import explain as X
from bpm_analysis_amd import reports as RP
from tests import beats_cases as C
from tests import test_beats as TB
from tests import test_beats_core as TBC
from tests import trace_cases as T

ROOT = os.path.dirname(T.HERE)
ROUTE_N = [12, 40, 63, 64, 65, 230, 605, 689]
ROUTE_SEEDS = [0, 1, 2]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("trace_core")


@pytest.fixture(scope="module")
def driver(workdir):
    exe = str(workdir / "trace_core_driver")
    b = T.build_driver(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    assert not b.stderr.strip(), b.stderr[-3000:]       # -Wall clean
    return exe


@pytest.fixture(scope="module")
def plain_driver(workdir):
    """beats_core_driver: the core without a trace."""
    exe = str(workdir / "beats_core_driver")
    import subprocess
    b = subprocess.run([T.cxx(), *T.BASE, "-o", exe, TBC.SRC], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def named():
    """[(name, table)]: the goldens that carry strings first, then the tables
    of the Python-route test."""
    gold = [(n, t) for n, g, t in C.golden_tables() if "info_vals" in g]
    route = [(f"n{n}_hint{h}", C.table(*C.craft(n, n), hint=h)) for n in C.SMALL_N for h in C.HINTS]
    route += [(f"n{n}_seed{s}_hint{h}", C.table(*C.craft(n, 10 * n + s), hint=h))
              for n in ROUTE_N for s in ROUTE_SEEDS for h in C.HINTS]
    route.append(("long", C.long_table()))
    return gold + route


@pytest.fixture(scope="module")
def case_file(workdir, named):
    path = str(workdir / "cases.bin")
    C.write_cases(path, [t for _, t in named])
    return path


@pytest.fixture(scope="module")
def traced(driver, workdir, case_file, named):
    return T.run_driver(driver, case_file, str(workdir / "out.bin"), str(workdir / "trace.bin"),
                        [t for _, t in named])


@pytest.fixture(scope="module")
def golden_data(named, traced):
    """{name: (golden, analysis_data from the driver's trace)}"""
    gold = {n: g for n, g, _ in C.golden_tables() if "info_vals" in g}
    assert len(gold) == 26
    out = {}
    for (name, t), tr in zip(named, traced[1]):
        if name in gold:
            out[name] = (gold[name], T.explain_table(t, tr))
    assert len(out) == 26
    return out


# ---- 1. goldens ----------------------------------------------------------------- #
def test_strings_equal_the_reference(golden_data):
    for name, (g, data) in golden_data.items():
        want = dict(zip((int(k) for k in g["info_keys"]), (str(v) for v in g["info_vals"])))
        got = {int(k): v for k, v in data["beat_debug_info"].items()}
        assert got.keys() == want.keys(), name
        for k in want:
            assert got[k] == want[k], (name, k)


def test_belief_and_deviation_equal_the_reference(golden_data):
    for name, (g, data) in golden_data.items():
        lt = data.get("long_term_bpm_series")
        if len(g["lt_t"]) == 0:
            assert lt is None, name
        else:
            assert np.asarray(lt.index, np.float64).tobytes() == np.asarray(g["lt_t"], np.float64).tobytes(), name
            assert np.asarray(lt.values, np.float64).tobytes() == np.asarray(g["lt_v"], np.float64).tobytes(), name
        dv = data["deviation_series"]
        assert np.asarray(dv.index, np.float64).tobytes() == np.asarray(g["dev_t"], np.float64).tobytes(), name
        assert np.asarray(dv.values, np.float64).tobytes() == np.asarray(g["dev_v"], np.float64).tobytes(), name


def test_trace_leaves_the_results_alone(plain_driver, workdir, case_file, named, traced):
    """Beats, tags, pass values and curves with the trace on equal those with it off."""
    tables = [t for _, t in named]
    plain = TBC._run(plain_driver, case_file, str(workdir / "plain.bin"), named)
    assert len(plain) == len(traced[0]) == len(tables)
    for (name, _), a, b in zip(named, plain, traced[0]):
        assert a["status"] == b["status"], name
        for k in ("final_peaks", "bpm_times", "bpm", "pass", "tags"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_staged_layout_gives_the_same_trace(driver, workdir, case_file, named, traced):
    tables = [t for _, t in named]
    _, staged = T.run_driver(driver, case_file, str(workdir / "out_s.bin"), str(workdir / "trace_s.bin"), tables,
                             "stage")
    for (name, _), a, b in zip(named, traced[1], staged):
        assert a["n_lt"] == b["n_lt"], name
        for k, _, _ in T.SLICES:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


# ---- 2. coverage ---------------------------------------------------------------- #
def test_goldens_contain_every_line_type(golden_data):
    """Every line the strings can have occurs in the compared goldens,
    including a gap correction nested five deep and a mixed S1-over-S2 nest."""
    text = [v for _, data in golden_data.values() for v in data["beat_debug_info"].values()]
    for piece in ("Stability Pre-Adjust", "PENALIZED by", "BOOSTED by", "Interval PENALTY by",
                  "Rejected Lone S1: Confidence", "Rejected Lone S1: Forward check failed", "Validated Lone S1",
                  "§First beat", "(Blended Model", ": nan\n", "-> Paired", "-> Not Paired"):
        assert any(piece in v for v in text), piece
    assert any(v == B.LONE_S1_LAST for v in text)
    assert any(v.startswith(B.LONE_S1_CASCADE) for v in text)
    assert any(v.startswith(B.S1_GAP) for v in text) and any(v.startswith(B.S2_GAP) for v in text)
    assert any(v.count(B.S1_GAP + "§ORIGINAL_REASON§") == 5 for v in text)
    assert any(B.S1_GAP in v and B.S2_GAP in v for v in text)


# ---- 3. the Python route --------------------------------------------------------- #
def test_explain_equals_the_python_route(named, traced):
    n_gold = sum(1 for n, g, _ in C.golden_tables() if "info_vals" in g)
    seen_gap = False
    for (name, t), res, tr in list(zip(named, *traced))[n_gold:]:
        data = T.explain_table(t, tr)
        if len(t["idx"]) < 2:
            with pytest.raises(KeyError):
                T.python_route(t)
            assert data == {"beat_debug_info": {}} and tr["n_lt"] == 0, name
            continue
        want = T.python_route(t)
        assert np.array_equal(res["final_peaks"], want["final_peaks"]), name
        T.assert_same_analysis(data, want["analysis_data"], name)
        seen_gap |= any(v.startswith(B.S1_GAP) for v in data["beat_debug_info"].values())
    assert seen_gap                                     # the 12 000-peak table's gap fill


# ---- 4. reports ------------------------------------------------------------------ #
def _packed_result(name, tr_used):
    """The per-file dict write_reports_packed takes, cut from the golden's
    whole arrays on the host; the metrics from beats.final_metrics."""
    g, params, hint, inp = TB.load_case(name)
    env = np.asarray(inp["env"], np.float64)
    flo = np.asarray(getattr(inp["floor"], "values", inp["floor"]), np.float64)
    pk, trg = np.asarray(inp["peaks"], np.int64), np.asarray(inp["troughs"], np.int64)
    data = X.assemble(pk, inp["sr"], params, tr_used, troughs=trg)
    return g, hint, dict(sr=inp["sr"], n_env=len(env), peaks=pk, env_pk=env[pk], floor_pk=flo[pk], troughs=trg,
                         env_tr=env[trg], floor_tr=flo[trg], analysis_data=data,
                         final_metrics=B.final_metrics(np.asarray(g["final_peaks"], np.int64), inp["sr"], params))


def test_reports_from_the_tables_equal_the_reference(named, traced, tmp_path):
    done = 0
    for (name, t), tr in zip(named, traced[1]):
        if name not in TB.CASES:
            continue
        g0 = np.load(os.path.join(TB.GOLD, "beats", name + ".npz"))
        if "summary_md" not in g0 or "info_vals" not in g0:
            continue
        g, hint, r = _packed_result(name, T.used(tr, len(t["idx"])))
        RP.write_reports_packed(os.path.join(str(tmp_path), name + ".wav"), str(tmp_path), r, hint)
        got = lambda suffix: (tmp_path / (name + suffix)).read_text(encoding="utf-8")  # noqa: E731
        assert TB._drop_stamp(got("_Analysis_Summary.md")) == str(g["summary_md"]), name
        assert TB._drop_stamp(got("_Debug_Log.md")) == str(g["debug_log_md"]), name
        assert got("_Analysis_Settings.json") == str(g["settings_json"]), name
        if str(g["csv"]):
            assert got("_bpm_plot.csv") == str(g["csv"]), name
        done += 1
    assert done == 26


# ---- 5. ABI ---------------------------------------------------------------------- #
def test_abi_of_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bpmx.h")).read()
    for name in ("bpmx_beats_device_ex", "bpmx_pack_trough_floor"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in N.EXPORTS
    assert "BPMX_ABI_VERSION 4" in re.sub(r"\s+", " ", hdr) and N.ABI_VERSION == 4
    assert ctypes.sizeof(N.TraceOut) == 64 and ctypes.sizeof(N.BeatsOut) == 64
    # the header's enums are the module's constants
    for cname, val in re.findall(r"\bBPMX_(TRF?_[A-Z0-9_]+) = (\d+)", hdr):
        assert getattr(N, cname) == int(val), cname
    assert N.TR_NFIELDS == 18


def test_null_arguments_give_e_arg():
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("libbpmx.so is not built")
    L = N.load()
    from bpm_analysis_amd import _host as H
    bp = H.beat_params(C.PARAMS)
    rc = L.bpmx_beats_device_ex(None, 1, C.SR, ctypes.byref(bp), 0.0, None, None, None, None, None, None)
    assert rc == N.E_ARG and b"bpmx_beats_device_ex" in L.bpmx_last_error()
    rc = L.bpmx_pack_trough_floor(None, None, None, 1, 1, None, None, None)
    assert rc == N.E_ARG and b"bpmx_pack_trough_floor" in L.bpmx_last_error()
    rc = L.bpmx_beats_device(None, 1, C.SR, ctypes.byref(bp), 0.0, None, None, None, None)
    assert rc == N.E_ARG and b"bpmx_beats_device:" in L.bpmx_last_error()


# ---- the sanitizer build ----------------------------------------------------------- #
def test_sanitizer_build_runs_clean(workdir, case_file, named, traced):
    exe = str(workdir / "trace_core_driver_san")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for link in (["-static-libasan", "-static-libubsan"], []):
        b = T.build_driver(exe, [*san, *link])
        if b.returncode == 0:
            break
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the sanitizer runtime does not link on this machine: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    tables = [t for _, t in named]
    for extra in ((), ("stage",)):
        res, trs = T.run_driver(exe, case_file, str(workdir / "out_san.bin"), str(workdir / "trace_san.bin"),
                                tables, *extra)
        for (name, _), a, b2, ta, tb in zip(named, traced[0], res, traced[1], trs):
            assert a["status"] == b2["status"] and a["final_peaks"].tobytes() == b2["final_peaks"].tobytes(), name
            assert ta["n_lt"] == tb["n_lt"], name
            for k, _, _ in T.SLICES:
                assert ta[k].tobytes() == tb[k].tobytes(), (name, k)
