"""bpmx_score_device (k_score) on the MI355X: label rows and reference tables
uploaded directly against ``labels.score`` with sentinels around every output,
both workspace routes, record-only launches, capacities one short; the beat
goldens through beats_device(trace=True), labels_device and score_device; the
settings sweep against the host route per setting; the drop-in entry point on
WAV files.  Integers are compared for equality."""
import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import beats_cases as C
from tests import labels_cases as LC
from tests import score_cases as SC
from tests import test_gpu_beats as G

pytestmark = pytest.mark.gpu

PAD = 8                                               # elements kept beyond every capacity
SLACK = (0, 3, 1, 0, 2)                               # label-row slices longer than n_labels, at odd offsets


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


# ---- 1. tables made directly --------------------------------------------------------------- #
def _launch(det, rows=True, cap=None, cap_ref=None):
    """bpmx_score_device on the shared cases' label rows and reference marks uploaded directly, every output
    filled with 0xFF bytes first -> host arrays, the two offset tables."""
    import torch
    dev = det.device
    cases = SC.cases()
    F = len(cases)
    marks = [LB.marks_from_table(ref) for _, _, ref in cases]
    nd = [4 if d is None else len(d["time"]) + SLACK[f % len(SLACK)] for f, (_, d, _) in enumerate(cases)]
    off = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(m["ms"]) for m in marks])]).astype(np.int64)
    tot, rtot = int(off[-1]), int(roff[-1])
    cap, cap_ref = tot if cap is None else cap, rtot if cap_ref is None else cap_ref
    lb_time, lb_type = np.full(tot + PAD, 1e9), np.full(tot + PAD, 7, np.int32)     # junk behind every n_labels
    n_labels, l_status = np.zeros(F, np.int32), np.zeros(F, np.int32)
    for f, (_, d, _) in enumerate(cases):
        if d is None:
            n_labels[f], l_status[f] = 3, N.LABELS_NONE   # a count that must not be read
            continue
        n = len(d["time"])
        lb_time[off[f]:off[f] + n], lb_type[off[f]:off[f] + n], n_labels[f] = d["time"], d["type"], n
    rf_ms = np.concatenate([m["ms"] for m in marks] + [np.full(PAD, -5, np.int32)]).astype(np.int32)
    rf_type = np.concatenate([m["type"] for m in marks] + [np.full(PAD, 1, np.int32)]).astype(np.int32)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    t = dict(lb_time=up(lb_time), lb_type=up(lb_type), n_labels=up(n_labels), l_status=up(l_status), off=up(off),
             roff=up(roff), rf_ms=up(rf_ms), rf_type=up(rf_type))
    ones = lambda n, dt: torch.full((n,), -1, dtype=dt, device=dev)  # noqa: E731
    out = dict(record=ones((F + PAD) * N.SCORE_RECORD, torch.int64), status=ones(F + PAD, torch.int32))
    if rows:
        out.update(sc_kind=ones(tot + PAD, torch.int32), sc_ref=ones(tot + PAD, torch.int32),
                   rf_kind=ones(rtot + PAD, torch.int32), rf_det=ones(rtot + PAD, torch.int32))
    k = N.PackedOut()
    k.cap_peaks, k.pk_off = cap, t["off"].data_ptr()
    lo = N.LabelsOut()
    lo.lb_time, lo.lb_type = t["lb_time"].data_ptr(), t["lb_type"].data_ptr()
    lo.n_labels, lo.status = t["n_labels"].data_ptr(), t["l_status"].data_ptr()
    r = N.RefMarks(cap_ref, t["roff"].data_ptr(), t["rf_ms"].data_ptr(), t["rf_type"].data_ptr())
    o = N.ScoreOut()
    for name in out:
        setattr(o, name, out[name].data_ptr())
    sp = N.ScoreParams(SC.TOL_MS, SC.GAP_MS)
    N.check(det.L.bpmx_score_device(det.ctx, F, ctypes.byref(sp), ctypes.byref(k), ctypes.byref(lo), ctypes.byref(r),
                                    ctypes.byref(o), det.stream_handle()), "bpmx_score_device")
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in out.items()}, off, roff


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(raw, off, roff, cap=None, cap_ref=None):
    """Every file against labels.score; everything no file owns against the sentinel."""
    cases, want = SC.cases(), SC.expected()
    F = len(cases)
    cap, cap_ref = int(off[-1]) if cap is None else cap, int(roff[-1]) if cap_ref is None else cap_ref
    rows = "sc_kind" in raw
    own_d = np.zeros(len(raw["sc_kind"]) if rows else 0, bool)
    own_r = np.zeros(len(raw["rf_kind"]) if rows else 0, bool)
    seen = set()
    for f, (name, d, _) in enumerate(cases):
        st = int(raw["status"][f])
        rec = raw["record"][f * N.SCORE_RECORD:(f + 1) * N.SCORE_RECORD]
        seen.add(st)
        if off[f + 1] > cap or roff[f + 1] > cap_ref:
            assert st == N.SCORE_OVERFLOW and _untouched(rec), name
            continue
        nd = 0 if d is None else len(d["time"])
        nr = int(roff[f + 1] - roff[f])
        got = {"status": st, "record": rec}
        if rows and st >= 0:
            a, ra = int(off[f]), int(roff[f])
            got.update(sc_kind=raw["sc_kind"][a:a + nd], sc_ref=raw["sc_ref"][a:a + nd],
                       rf_kind=raw["rf_kind"][ra:ra + nr], rf_det=raw["rf_det"][ra:ra + nr])
            own_d[a:a + nd] = True
            own_r[ra:ra + nr] = True
        SC.assert_same(got, want[f], name)
        SC.check_identities(rec, nd)
    if rows:
        for k, own in (("sc_kind", own_d), ("sc_ref", own_d), ("rf_kind", own_r), ("rf_det", own_r)):
            assert _untouched(raw[k][~own]), f"{k}: a write outside the files' used entries"
    assert _untouched(raw["status"][F:]) and _untouched(raw["record"][F * N.SCORE_RECORD:])
    return seen


def test_direct_tables_equal_labels_py(det):
    raw, off, roff = _launch(det)
    assert _check(raw, off, roff) == {N.SCORE_OK, N.SCORE_NO_LABELS, N.SCORE_NONE}
    st = {n: int(raw["status"][f]) for f, (n, _, _) in enumerate(SC.cases())}
    assert (st["no_labels"], st["no_ref"], st["no_labels_no_ref"], st["no_det"]) == \
        (N.SCORE_NO_LABELS, N.SCORE_NONE, N.SCORE_NONE, N.SCORE_OK)
    assert sum(int(o) % 2 for o in off[:-1]) >= 3 and sum(int(o) % 2 for o in roff[:-1]) >= 3   # slices at odd offsets


def test_both_workspace_routes_give_the_same(det):
    plain, off, roff = _launch(det)
    det.set_options(N.OPT_SCORE_GLOBAL)
    try:
        forced, _, _ = _launch(det)
    finally:
        det.set_options(0)
    _check(forced, off, roff)
    for k in plain:
        assert plain[k].tobytes() == forced[k].tobytes(), k


@pytest.mark.parametrize("options", [0, N.OPT_SCORE_GLOBAL])
def test_record_only(det, options):
    det.set_options(options)
    try:
        raw, off, roff = _launch(det, rows=False)
    finally:
        det.set_options(0)
    assert sorted(raw) == ["record", "status"]
    assert _check(raw, off, roff) == {N.SCORE_OK, N.SCORE_NO_LABELS, N.SCORE_NONE}


def test_capacities_one_short(det):
    """The last recording's slice reaches past the capacity: OVERFLOW, nothing else touched."""
    _, off, roff = _launch(det, rows=False)
    last = len(SC.cases()) - 1
    for cap, cap_ref in ((int(off[-1]) - 1, None), (None, int(roff[-1]) - 1)):
        raw, _, _ = _launch(det, cap=cap, cap_ref=cap_ref)
        seen = _check(raw, off, roff, cap=cap, cap_ref=cap_ref)
        assert N.SCORE_OVERFLOW in seen and int(raw["status"][last]) == N.SCORE_OVERFLOW
        assert [int(s) for s in raw["status"][:last]].count(N.SCORE_OVERFLOW) == 0
        assert _untouched(raw["sc_kind"][int(off[last]):]) and _untouched(raw["rf_det"][int(roff[last]):])


# ---- 2. the beat goldens through beats, labels and score ---------------------------------- #
def test_goldens_through_beats_labels_and_score(det):
    import torch
    fx = {n: f for n, f, _ in LC.golden_cases()}
    groups = {}
    for name, g, t in C.golden_tables():
        groups.setdefault((bytes(H.beat_params(t["params"])), t["hint"], t["sr"]), []).append((name, t))
    n_same = n_none = 0
    kinds = np.zeros(4, np.int64)
    for members in groups.values():
        tables = [t for _, t in members]
        b = det.beats_device(G._upload(det, tables), tables[0]["params"], tables[0]["hint"], trace=True)
        lab = det.labels_device(b, 5.0)
        host = lab.to_host()
        fixture = [LC.expected(fx[name], 5.0) for name, _ in members]
        same = [None if w is None else w["table"] for w in fixture]
        moved = [None if w is None else SC.corrected(w["table"], 40 + f, spans=2) for f, w in enumerate(fixture)]
        for refs in (same, moved):
            sc = det.score_device(lab, det.upload_marks(refs), SC.TOL_SEC, SC.GAP_SEC)
            got = sc.to_host()
            rec_only = det.score_device(lab, sc.marks, SC.TOL_SEC, SC.GAP_SEC, rows=False).to_host()
            torch.cuda.synchronize()
            for f, (name, _) in enumerate(members):
                tab = None if host[f] is None else host[f]["table"]
                want = LB.score(tab, refs[f], SC.TOL_SEC, SC.GAP_SEC)
                SC.assert_same(got[f], want, name)
                SC.assert_same(rec_only[f], want, name)
                assert "sc_kind" not in rec_only[f]
                if refs is same and tab is not None:
                    n1, n2 = int((tab["type"] == 1).sum()), int((tab["type"] == 2).sum())
                    assert got[f]["status"] == N.SCORE_OK, name
                    assert got[f]["record"].tolist() == [n1, n1, n1, 0, 0, 0, 0, 0, 0, n2, n2, n2, 0, 0, 0, 0, 0, 0, 0,
                                                          int(got[f]["record"][N.SR_N_SPANS])], name
                    assert set(got[f]["sc_kind"].tolist()) == {N.SCORE_TP}, name
                    n_same += 1
                elif refs is same:
                    assert got[f]["status"] == N.SCORE_NONE and got[f]["record"].tolist() == [0] * 20, name
                    n_none += 1
                else:
                    kinds += np.bincount(got[f]["sc_kind"], minlength=4)[:4]
    assert n_same == 26 and n_none == 2
    assert kinds.min() > 20                               # outside, TP, SWAP and FP all occur among the moved marks


# ---- 3. the settings sweep ------------------------------------------------------------------ #
SWEEP_SECS = (20, 23, 27, 31, 36, 40)


@pytest.fixture(scope="module")
def sweep_inputs():
    fs = 44100
    recs = []
    for k, secs in enumerate(SWEEP_SECS):
        out = np.zeros(secs * fs + 17 * k, np.int16)
        N.load().bpmx_synth_host(900 + k, len(out), fs, 1, out.ctypes.data)
        recs.append(out)
    base = dict(C.PARAMS)
    grid = [base,
            dict(base, min_peak_distance_sec=0.2, noise_floor_quantile=0.5),
            dict(base, pairing_confidence_threshold=float(base["pairing_confidence_threshold"]) * 1.4,
                 trough_rejection_multiplier=2.0),
            dict(base, min_peak_distance_sec=0.03, noise_floor_quantile=0.1, trough_rejection_multiplier=6.0)]
    return fs, recs, grid


def test_sweep_equals_the_host_route_per_setting(det, sweep_inputs):
    fs, recs, grid = sweep_inputs
    tol, gap = 0.05, 5.0
    host = [det.run_host_reports(recs, fs, p, mode="reference", labels=True, label_gap_sec=gap) for p in grid]
    tables = [[None if r.get("labels") is None else r["labels"]["table"] for r in res] for res in host]
    assert all(t is not None and len(t["time"]) > 20 for t in tables[0])
    refs = [SC.corrected(t, 70 + f) for f, t in enumerate(tables[0])]         # the first setting's marks, corrected
    want = np.array([[LB.score(t, ref, tol, gap)["record"] for t, ref in zip(ts, refs)] for ts in tables])
    # the settings matter, on the host route already: otherwise the comparison below shows nothing
    assert any((want[p] != want[q]).any() for p in range(len(grid)) for q in range(p))
    det.profile_only("")
    det.profile(True)
    rec, status = det.score_sweep(recs, fs, grid, refs, mode="reference", tol_sec=tol, gap_sec=gap)
    det.profile(False)
    sweep_prof = det.profile_read()
    assert rec.shape == (len(grid), len(recs), N.SCORE_RECORD) and rec.dtype == np.int64
    assert status.shape == (len(grid), len(recs)) and (status == N.SCORE_OK).all()
    assert rec.tolist() == want.tolist()
    # the envelope was made once: its kernels were launched as often as in one envelope-stage run, not per setting
    import torch
    fo = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate(recs)).to(det.device)
    det.profile(True)
    res = det.run(pcm, fo, fs, grid[0], mode="reference", stages=N.STAGE_ENVELOPE)
    det.profile(False)
    env_prof = det.profile_read()
    det.profile(True)
    det.run(None, fo, fs, grid[0], mode="reference", stages=N.STAGE_FLOOR | N.STAGE_PEAKS, out=res)
    det.profile(False)
    det_prof = det.profile_read()
    env_only = sorted(set(env_prof) - set(det_prof))
    assert env_only and all(k in sweep_prof for k in env_only)
    assert {k: sweep_prof[k][0] for k in env_only} == {k: env_prof[k][0] for k in env_only}
    assert sweep_prof["k_score"][0] == len(grid) and sweep_prof["k_labels"][0] == len(grid)


def test_sweep_rejects_settings_with_different_envelopes(det, sweep_inputs):
    fs, recs, grid = sweep_inputs
    det.profile(True)
    with pytest.raises(ValueError, match="downsample_factor"):
        det.score_sweep(recs[:2], fs, [grid[0], dict(grid[0], downsample_factor=100)], [None, None])
    det.profile(False)
    assert det.profile_read() == {}                       # before anything runs


# ---- 4. the drop-in entry point -------------------------------------------------------------- #
E2E = [dict(seed=51, secs=9, fs=44100), dict(seed=52, secs=11, fs=44100), dict(seed=53, secs=12, fs=44100),
       dict(seed=54, secs=8, fs=44100)]


def _edit(path, seed):
    """A person's corrections: marks removed, moved within and beyond the tolerance, and renamed."""
    rng = np.random.default_rng(seed)
    t = LB.read_labels(path)
    n = len(t["time"])
    assert n > 12
    keep = np.ones(n, bool)
    keep[rng.choice(n, 2, replace=False)] = False
    time, typ = t["time"].copy(), t["type"].copy()
    time[3] += 0.03
    time[5] -= 0.12
    typ[7] = 3 - typ[7]
    tab = LB._table(t["pos"][keep], typ[keep], np.round(time[keep], 3), t["bpm"][keep])
    assert LB.write_labels(path, LB.analyse(tab), overwrite=True)


def test_score_wav_files_equals_the_host_route(tmp_path):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin as D
    from tests.golden import inputs as I
    src = tmp_path / "src"
    src.mkdir()
    paths = []
    for k, spec in enumerate(E2E):
        pcm, fs = I.make_input(spec)
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
    base = dict(C.PARAMS, save_filtered_wav=True)
    grid = [dict(base, save_filtered_wav=False), dict(base, save_filtered_wav=False, min_peak_distance_sec=0.09,
                                                      noise_floor_quantile=0.3)]
    first = D.analyze_wav_files_to_reports(paths, base, str(src), mode="native", labels=True)
    assert all("error" not in r and r["labels_written"] for r in first)
    label_paths = [LB.labels_path(p, str(src)) for p in paths]
    for k, lp in enumerate(label_paths[:3]):
        _edit(lp, 80 + k)
    os.remove(label_paths[3])                             # a file nobody labelled
    filtered = [f"{os.path.splitext(p)[0]}_filtered_debug.wav" for p in paths]
    assert all(os.path.exists(p) for p in filtered)
    refs = [LB.read_labels(lp) for lp in label_paths[:3]]
    for mode, files, lps in (("native", paths, None), ("rectified", filtered, label_paths)):
        got = D.score_wav_files(files, grid, label_paths=lps, mode=mode)
        assert len(got) == len(grid)
        for p, params in enumerate(grid):
            out = tmp_path / f"host_{mode}_{p}"
            out.mkdir()
            res = D.analyze_wav_files_to_reports(files[:3], params, str(out), mode=mode, labels=True)
            recs = [LB.score(None if r.get("labels") is None else r["labels"]["table"], ref)["record"]
                    for r, ref in zip(res, refs)]
            g = got[p]
            assert g["params"] == params
            for k in range(3):
                assert g["files"][k]["record"].tolist() == recs[k].tolist(), (mode, p, k)
                assert g["files"][k]["status"] == N.SCORE_OK and g["files"][k]["all"]["tp"] > 5
                assert g["files"][k]["S1"] == LB.score_summary(recs[k])["S1"]
            assert isinstance(g["files"][3]["error"], FileNotFoundError)
            tot = LB.score_total(recs)
            assert g["total"]["record"].tolist() == tot.tolist() and g["total"]["n_files"] == 3
            assert g["total"]["all"]["recall"] == LB.score_summary(tot)["all"]["recall"] < 1.0
            assert tot[N.SR_FN] + tot[N.SR_PER_TYPE + N.SR_FN] + tot[N.SR_SWAP] + tot[N.SR_PER_TYPE + N.SR_SWAP] > 0
