"""Shared by test_trace_core.py (CPU) and test_gpu_trace.py: the binary exchange
with trace_core_driver, the per-file trace dicts ``explain`` takes, and the
Python route (``beats.analyze_recording`` on NaN-scratch arrays) they are
compared with."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from bpm_analysis_amd import explain as X
from tests import beats_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "trace_core_driver.cpp")
BASE = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall"]
NF = N.TR_NFIELDS
# (name, dtype, entries per raw peak) of a recording's trace slices, in the driver's file order
SLICES = (("record", np.float64, NF), ("code", np.int32, 1), ("lt_pos", np.int32, 1), ("lt_bpm", np.float64, 1),
          ("dev_t", np.float64, 1), ("dev", np.float64, 1), ("gap", np.int32, 1))


def cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"


def build_driver(exe, extra=()):
    return subprocess.run([cxx(), *BASE, *extra, "-o", exe, SRC], capture_output=True, text=True, timeout=600)


def run_driver(exe, case_file, out, trace, tables, *extra):
    """-> (results as beats_cases.read_results, whole trace slices per table)"""
    r = subprocess.run([exe, case_file, out, trace, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    return C.read_results(out, tables), read_traces(trace, tables)


def read_traces(path, tables):
    """Per table: n_lt and every slice whole (n entries; what the core left
    alone is 0xFF bytes), as the device keeps them."""
    buf = open(path, "rb").read()
    o, out = 0, []
    for t in tables:
        n = len(t["idx"])
        d = dict(n_lt=int(np.frombuffer(buf, np.int32, 1, o)[0]))
        o += 4
        for name, dt, per in SLICES:
            d[name] = np.frombuffer(buf, dt, n * per, o)
            o += n * per * np.dtype(dt).itemsize
        out.append(d)
    assert o == len(buf)
    return out


def used(tr, n):
    """The slices ``explain.assemble`` reads: the valid prefixes."""
    nd = max(n - 1, 0)
    return dict(record=tr["record"].reshape(n, NF), code=tr["code"], gap=tr["gap"], lt_pos=tr["lt_pos"][:tr["n_lt"]],
                lt_bpm=tr["lt_bpm"][:tr["n_lt"]], dev_t=tr["dev_t"][:nd], dev=tr["dev"][:nd])


def python_route(t):
    """``beats.analyze_recording`` on a table (env and floor NaN except at the
    raw peaks, as _host.beats_packed runs the host library)."""
    idx = t["idx"].astype(np.int64)
    n_env = int(idx[-1]) + 1 if len(idx) else 0
    env, flo = np.full(n_env, np.nan), np.full(n_env, np.nan)
    env[idx], flo[idx] = t["env"], t["flo"]
    return B.analyze_recording(env, t["sr"], flo, np.zeros(0, np.int64), idx, t["params"], t["hint"])


def same_series(a, b):
    """Two pd.Series bit for bit, index included."""
    av, bv = np.asarray(a.values, np.float64), np.asarray(b.values, np.float64)
    ai, bi = np.asarray(a.index, np.float64), np.asarray(b.index, np.float64)
    return av.tobytes() == bv.tobytes() and ai.tobytes() == bi.tobytes()


def assert_same_analysis(data, want, what=""):
    """analysis_data of ``explain.assemble`` against the Python route's."""
    assert data["beat_debug_info"] == want["beat_debug_info"], what
    assert list(data["beat_debug_info"]) == list(want["beat_debug_info"]) or \
        sorted(data["beat_debug_info"]) == sorted(want["beat_debug_info"]), what
    assert ("long_term_bpm_series" in data) == ("long_term_bpm_series" in want), what
    if "long_term_bpm_series" in want:
        assert same_series(data["long_term_bpm_series"], want["long_term_bpm_series"]), what
    assert same_series(data["deviation_series"], want["deviation_series"]), what


def explain_table(t, tr):
    return X.assemble(t["idx"], t["sr"], t["params"], used(tr, len(t["idx"])))
