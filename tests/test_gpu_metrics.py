"""bpmx_metrics_device (csrc/k_metrics.hip) on the MI355X: the final metrics
from the beats and curves where bpmx_beats_device leaves them.  Two targets:
tests/metrics_core_driver.cpp (the same core on the CPU) on exactly the beats
and curve the kernel read, and ``beats.final_metrics``' parts on that curve.
Positions, counts and status equal, doubles within TB.RTOL; the tests record
whether the doubles were bit-identical.  Every output is pre-filled with
sentinels: nothing outside a file's counts or beyond the capacity is written."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from tests import beats_cases as C
from tests import metrics_cases as M
from tests import test_gpu_beats as GB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
I32_S, F64_S = GB.I32_S, GB.F64_S
ROWS_F = ("hrv_time", "hrv_rmssdc", "hrv_sdnn", "hrv_bpm", "inc_slope", "inc_dur", "dec_slope", "dec_dur")
ROWS_I = ("inc_a", "inc_b", "dec_a", "dec_b")
OWNER = dict(hrv_time="n_hrv", hrv_rmssdc="n_hrv", hrv_sdnn="n_hrv", hrv_bpm="n_hrv", inc_a="n_inc", inc_b="n_inc",
             inc_slope="n_inc", inc_dur="n_inc", dec_a="n_dec", dec_b="n_dec", dec_slope="n_dec", dec_dur="n_dec")


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    """cases -> the CPU driver's results."""
    work = tmp_path_factory.mktemp("gpu_metrics")
    exe = str(work / "metrics_core_driver")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
    b = subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-o", exe,
                        os.path.join(HERE, "metrics_core_driver.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    count = [0]

    def run(cases):
        count[0] += 1
        inp, out = str(work / f"in{count[0]}.bin"), str(work / f"out{count[0]}.bin")
        M.write_cases(inp, cases)
        r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
        return M.read_results(out, len(cases))
    return run


def _packed(det, off, cap, sr, flags=None):
    import torch
    from bpm_analysis_amd.engine import Packed
    F, dev = len(off) - 1, det.device
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    return Packed(det=det, sr=sr, doff=np.zeros(F + 1, np.int64), cap_peaks=cap, cap_troughs=0,
                  safe_peaks=int(off[-1]), safe_troughs=0, pk_off=torch.from_numpy(np.asarray(off, np.int64)).to(dev),
                  tr_off=z, pk_idx=None, pk_env=None, pk_floor=None, tr_idx=None, tr_env=None, y16=None, y_max=None,
                  flags=flags)


def _upload_beats(det, cases, slack):
    """A Beats on the device holding these cases' final beats and curves, file
    f's slice `slack[f]` entries longer than its beats."""
    import torch
    from bpm_analysis_amd.engine import Beats
    n = [len(c["fin"]) + s for c, s in zip(cases, slack)]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    cap, F, dev = int(off[-1]), len(cases), det.device
    fin = np.full(cap + 8, I32_S, np.int32)
    bt, bv = np.full(cap + 8, F64_S), np.full(cap + 8, F64_S)
    for c, a in zip(cases, off):
        fin[a:a + len(c["fin"])] = c["fin"]
        bt[a:a + len(c["bt"])] = c["bt"]
        bv[a:a + len(c["bv"])] = c["bv"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pk = _packed(det, off, cap, cases[0]["sr"])
    b = Beats(det=det, packed=pk, final_idx=up(fin), n_final=up(np.array([len(c["fin"]) for c in cases], np.int32)),
              bpm_t=up(bt), bpm=up(bv), n_bpm=up(np.array([len(c["bt"]) for c in cases], np.int32)), pass_=None,
              tags=None, status=up(np.array([c["bst"] for c in cases], np.int32)))
    return b, off


def _metrics(det, beats, params, epoch_s=0):
    """bpmx_metrics_device with every output filled with sentinels first -> host arrays."""
    import torch
    pk = beats.packed
    F, cap, dev = pk.n_files, max(int(pk.cap_peaks), 1), det.device
    full = lambda n, v, dt: torch.full((n + 8,), v, dtype=dt, device=dev)  # noqa: E731
    t = {k: full(cap, F64_S, torch.float64) for k in ROWS_F}
    t.update({k: full(cap, I32_S, torch.int32) for k in ROWS_I})
    t.update({k: full(F, I32_S, torch.int32) for k in ("n_hrv", "n_inc", "n_dec", "status")})
    t["record"] = full(F * N.METRICS_RECORD, F64_S, torch.float64)
    k = N.PackedOut()
    k.cap_peaks, k.pk_off = pk.cap_peaks, pk.pk_off.data_ptr()
    b = N.BeatsOut()
    b.final_idx, b.n_final, b.bpm_t, b.bpm = (x.data_ptr() for x in (beats.final_idx, beats.n_final, beats.bpm_t,
                                                                      beats.bpm))
    b.n_bpm, b.status = beats.n_bpm.data_ptr(), beats.status.data_ptr()
    o = N.MetricsOut()
    for name, _ in N.MetricsOut._fields_:
        setattr(o, name, t[name].data_ptr())
    mp = N.metric_params(params)
    N.check(det.L.bpmx_metrics_device(det.ctx, F, int(pk.sr), ctypes.byref(mp), int(epoch_s) * 1000000,
                                      ctypes.byref(k), ctypes.byref(b), ctypes.byref(o), det.stream_handle()),
            "bpmx_metrics_device")
    torch.cuda.synchronize()
    return {name: x.cpu().numpy() for name, x in t.items()}


def _file(raw, f, a):
    nh, ni, nd = (int(raw[k][f]) for k in ("n_hrv", "n_inc", "n_dec"))
    R = N.METRICS_RECORD
    return dict(status=int(raw["status"][f]), record=raw["record"][R * f:R * f + R],
                hrv={c: raw["hrv_" + c][a:a + nh] for c in M.HRV_COLS},
                inc={c: raw["inc_" + c][a:a + ni] for c in M.RUN_COLS},
                dec={c: raw["dec_" + c][a:a + nd] for c in M.RUN_COLS})


def _check_batch(raw, cases, off, want_cpu, cap=None, host=True):
    """Every file against the CPU driver (and the host functions), every
    element no file owns against its sentinel -> doubles bit-identical?"""
    F = len(cases)
    cap = int(off[-1]) if cap is None else cap
    used = {k: np.zeros(len(raw[k]), bool) for k in OWNER}
    bits = True
    R = N.METRICS_RECORD
    for f, c in enumerate(cases):
        a, n = int(off[f]), int(off[f + 1] - off[f])
        if a + n > cap:
            assert raw["status"][f] == N.METRICS_OVERFLOW, f
            assert all(raw[k][f] == I32_S for k in ("n_hrv", "n_inc", "n_dec")), f
            assert (raw["record"][R * f:R * f + R] == F64_S).all(), f
            continue
        got = _file(raw, f, a)
        for k, own in OWNER.items():
            assert 0 <= raw[own][f] <= n, (f, own)
            used[k][a:a + int(raw[own][f])] = True
        w = want_cpu[f]
        assert got["status"] == w["status"], (f, got["status"], w["status"])
        bits &= M.assert_same(got, w, f"file {f} against the CPU core", bits=False)
        if host:
            M.check(got, c, f"file {f} against the host", bits=False)
    for k in OWNER:
        s = I32_S if k in ROWS_I else F64_S
        assert (raw[k][~used[k]] == s).all(), f"{k}: a write outside the files' counts"
    for k in ("n_hrv", "n_inc", "n_dec", "status"):
        assert (raw[k][F:] == I32_S).all(), k
    assert (raw["record"][R * F:] == F64_S).all()
    return bits


def _groups(named):
    """Cases that share parameters, rate and epoch share a launch."""
    g = {}
    for name, c in named:
        p = c["params"]
        key = (p["hrv_window_size_beats"], p["hrv_step_size_beats"], c["sr"], c["epoch_s"])
        g.setdefault(key, []).append((name, c))
    return list(g.values())


def _crafted_groups():
    groups = _groups(M.crafted_cases())
    main = max(groups, key=len)
    empty = M.case(np.zeros(0, np.int32))
    main.insert(0, ("empty_front", empty))
    main.append(("empty_back", empty))
    return groups


def test_crafted_batches(det, cpu, record_property):
    """Final-beat counts 0 ... 605 with the 39 / 40 / 41 beat and 64 / 65 window
    cases, empty files at both ends, batches of one file among them; then
    every file forced onto the global path, which must give the same bytes."""
    groups = _crafted_groups()
    assert len(max(groups, key=len)) >= 24 and any(len(g) == 1 for g in groups)
    counts = sorted(len(c["fin"]) for g in groups for _, c in g)
    assert counts[0] == 0 and 605 in counts and counts[-1] <= 720      # all within the LDS budget by size
    bits = True
    for g in groups:
        cases = [c for _, c in g]
        slack = [(3 * f) % 5 for f in range(len(cases))]
        beats, off = _upload_beats(det, cases, slack)
        want = cpu(cases)
        raw = _metrics(det, beats, cases[0]["params"], cases[0]["epoch_s"])
        bits &= _check_batch(raw, cases, off, want)
        det.set_options(N.OPT_METRICS_GLOBAL)
        try:
            glob = _metrics(det, beats, cases[0]["params"], cases[0]["epoch_s"])
        finally:
            det.set_options(0)
        for k in raw:
            assert raw[k].tobytes() == glob[k].tobytes(), (g[0][0], k)
    record_property("doubles_bit_identical", bits)
    print("doubles bit-identical:", bits)


def test_tie_bit_on_the_device(det, cpu, record_property):
    named = M.tie_cases()
    cases = [c for _, c in named]
    beats, off = _upload_beats(det, cases, [0] * len(cases))
    want = cpu(cases)
    raw = _metrics(det, beats, M.PARAMS)
    bits = _check_batch(raw, cases, off, want, host=False)
    flagged = sum(int(w["status"]) == N.METRICS_TIE for w in want)
    assert 0.1 * len(cases) <= flagged <= 0.9 * len(cases)
    record_property("doubles_bit_identical", bits)


def _beats_then_metrics(det, tables, cap=None, flags=None, params=None, hint=None):
    """bpmx_beats_device on a packed table, then bpmx_metrics_device on its
    outputs -> (raw metrics, the cases the kernel read, offsets)."""
    import torch
    from bpm_analysis_amd.engine import Beats
    params = params or C.PARAMS
    pk = GB._upload(det, tables, cap=cap, flags=flags)
    b = det.beats_device(pk, params, hint)
    torch.cuda.synchronize()
    off = GB._offsets(tables)
    h = {k: getattr(b, k).cpu().numpy() for k in ("final_idx", "n_final", "bpm_t", "bpm", "n_bpm", "status")}
    cases = []
    for f, t in enumerate(tables):
        a = int(off[f])
        if a + len(t["idx"]) > int(pk.cap_peaks):
            cases.append(M.case(np.zeros(0, np.int32), sr=t["sr"], params=params))
            continue
        nf, nb = int(h["n_final"][f]), int(h["n_bpm"][f])
        cases.append(M.case(h["final_idx"][a:a + nf], sr=t["sr"], params=params, bst=int(h["status"][f]),
                            curve=(h["bpm_t"][a:a + nb], h["bpm"][a:a + nb])))
    assert isinstance(b, Beats)
    return _metrics(det, b, params), cases, off, int(pk.cap_peaks)


def test_behind_the_beats_kernel(det, cpu):
    tables = GB._crafted()
    raw, cases, off, _ = _beats_then_metrics(det, tables)
    _check_batch(raw, cases, off, cpu(cases))
    assert sum(r >= 0 for r in raw["status"][:len(tables)]) >= 8


def test_long_table_takes_the_global_path(det, cpu, record_property):
    t = C.long_table()
    assert len(t["idx"]) == 12000
    raw, cases, off, _ = _beats_then_metrics(det, [t])
    assert len(cases[0]["fin"]) > 3000
    bits = _check_batch(raw, cases, off, cpu(cases))
    assert raw["n_hrv"][0] > 500
    record_property("doubles_bit_identical", bits)


def test_capacity_smaller_than_the_total(det, cpu):
    tables = GB._crafted()
    off = GB._offsets(tables)
    cap = int(off[14]) + 20
    raw, cases, off, cap = _beats_then_metrics(det, tables, cap=cap)
    _check_batch(raw, cases, off, cpu(cases), cap=cap)
    st = raw["status"][:len(tables)]
    assert (st[14:] == N.METRICS_OVERFLOW).all() and (st[:14] != N.METRICS_OVERFLOW).all()


def test_flagged_file_has_no_metrics(det, cpu):
    tables = GB._crafted()
    flags = np.zeros(len(tables), np.int32)
    flags[12] = N.F_TOO_SHORT
    raw, cases, off, _ = _beats_then_metrics(det, tables, flags=flags)
    assert cases[12]["bst"] == N.BEATS_SKIPPED and raw["status"][12] == N.METRICS_NONE
    _check_batch(raw, cases, off, cpu(cases))


def test_golden_cases_against_the_recorded_metrics(det, cpu):
    """The goldens through both kernels, against the reference's own recorded
    metrics (the bars of test_beats.check_against_golden)."""
    import json

    from bpm_analysis_amd import _host as H
    from bpm_analysis_amd import metrics as MH
    from tests import test_beats as TB
    groups = {}
    for name, g, t in C.golden_tables():
        if "metrics" in g:
            key = (bytes(H.beat_params(t["params"])), bytes(N.metric_params(t["params"])), t["hint"], t["sr"])
            groups.setdefault(key, []).append((name, g, t))
    assert sum(len(v) for v in groups.values()) == 26
    for members in groups.values():
        tables = [t for _, _, t in members]
        raw, cases, off, _ = _beats_then_metrics(det, tables, params=tables[0]["params"], hint=tables[0]["hint"])
        _check_batch(raw, cases, off, cpu(cases))
        for f, (name, g, t) in enumerate(members):
            got, c = _file(raw, f, int(off[f])), cases[f]
            assert got["status"] in (N.METRICS_OK, N.METRICS_TIE), name
            with M.epoch(0):
                m = MH.assemble(c["bt"], c["bv"], got["record"], got["hrv"], got["inc"], got["dec"])
            assert np.array_equal(m["smoothed_bpm"].index.asi8, g["bpm_ns"]), name
            for col in M.HRV_COLS:
                h = m["windowed_hrv_df"]
                TB._close(h[col].to_numpy(float) if len(h) else np.zeros(0), g["hrv_" + col], f"{name} hrv {col}")
            ref = json.loads(str(g["metrics"]))
            if got["status"] == N.METRICS_OK:
                for k in ("major_inclines", "major_declines"):
                    assert len(m[k]) == len(ref[k]), (name, k)
                    for i, (o, r) in enumerate(zip(m[k], ref[k])):
                        TB._cmp_obj(o, r, f"{name} {k}[{i}]")
            for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
                TB._cmp_obj(m[k], ref[k], f"{name} {k}")
            assert list(m["hrv_summary"]) == list(ref["hrv_summary"]), name
            for k, v in ref["hrv_summary"].items():
                TB._close(m["hrv_summary"][k], v, f"{name} hrv_summary {k}")


@pytest.mark.parametrize("mode", ["native", "reference"])
def test_run_host_metrics_end_to_end(det, mode):
    """PCM in, per-file dicts with final_metrics out, against run_host_beats
    and beats.final_metrics on its beats."""
    import pandas as pd

    from bpm_analysis_amd import beats as B
    from oracle import oracle as O
    recs = [O.synth(60 + i, n, 44100, 1) for i, n in enumerate(GB.FRAMES)]
    got = det.run_host_metrics(recs, 44100, C.PARAMS, mode=mode)
    base = det.run_host_beats(recs, 44100, C.PARAMS, mode=mode)
    assert len(got) == len(base) == len(recs)
    n = 0
    for f, (g, b) in enumerate(zip(got, base)):
        assert g["metrics_source"] in ("device", "host")
        GB._same_dict({k: v for k, v in g.items() if k not in ("final_metrics", "metrics_source")}, b, f"file {f}")
        if "final_peaks" not in b or len(b["final_peaks"]) < 2:
            assert g["final_metrics"] is None, f
            continue
        m, want = g["final_metrics"], B.final_metrics(b["final_peaks"], 302, C.PARAMS)
        assert list(m) == list(want), f
        assert np.array_equal(m["smoothed_bpm"].index.asi8, want["smoothed_bpm"].index.asi8), f
        np.testing.assert_allclose(m["smoothed_bpm"].values, want["smoothed_bpm"].values, rtol=C.TB.RTOL, atol=0)
        assert list(m["hrv_summary"]) == list(want["hrv_summary"]), f
        for k, v in want["hrv_summary"].items():
            np.testing.assert_allclose(m["hrv_summary"][k], v, rtol=C.TB.RTOL, atol=0)
        for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
            assert (m[k] is None) == (want[k] is None), (f, k)
            for q, v in (want[k] or {}).items():
                if isinstance(v, pd.Timestamp):
                    assert m[k][q] == v, (f, k, q)
                else:
                    np.testing.assert_allclose(m[k][q], v, rtol=C.TB.RTOL, atol=0)
        assert len(m["windowed_hrv_df"]) == len(want["windowed_hrv_df"]), f
        for k in ("major_inclines", "major_declines"):
            assert len(m[k]) == len(want[k]), (f, k)
        n += 1
    assert n >= 2 and got[2].get("skipped") is True


def test_run_sharded_device_metrics_equal_the_host_fallback(det):
    """run_sharded(beats="device", metrics=True): the records come from
    bpmx_metrics_device; with beats="native" final_metrics runs on the host."""
    from bpm_analysis_amd.shard import run_sharded
    from oracle import oracle as O
    recs = [O.synth(60 + i, n, 44100, 1) for i, n in enumerate(GB.FRAMES)]
    kw = dict(fs=44100, mode="native", detector=det, host_threads=2, chunk_frames=44100 * 20)
    a = run_sharded(recs, C.PARAMS, beats="native", metrics=True, **kw)
    b = run_sharded(recs, C.PARAMS, beats="device", metrics=True, **kw)
    plain = run_sharded(recs, C.PARAMS, beats="device", **kw)
    assert len(a) == len(b) == len(plain) == len(recs)
    for f, (x, y, p) in enumerate(zip(a, b, plain)):
        GB._same_dict(y, x, f"file {f}")
        assert "metrics_record" not in p and "n_hrv" not in p
        GB._same_dict({k: v for k, v in y.items() if k not in ("metrics_record", "n_hrv")}, p, f"file {f}")
        if "error" not in y:
            pos = list(M.POSITIONS)
            assert np.array_equal(x["metrics_record"][pos], y["metrics_record"][pos], equal_nan=True), f
    assert isinstance(b[2]["error"], ValueError) and not np.isnan(b[0]["metrics_record"][N.MR_AVG_BPM])
