"""bpmx_marks_device (k_marks) on the MI355X: the shared mark tables uploaded
directly against ``labels.rows_from_marks`` / ``beats.bpm_series`` with 0xFF
bytes around every output and an odd capacity, both workspace routes,
capacities below the total and a descending rf_off; the chain through
metrics_device, labels_device and score_device against ``labels.revise`` /
``labels.score`` and the reference-made goldens; the closed loop from an
analysis' own label tables; the drop-in entry points on files.  Integers are
compared for equality, doubles as bit patterns."""
import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import beats_cases as C
from tests import marks_cases as MC
from tests import metrics_cases as M
from tests import test_marks as TM

pytestmark = pytest.mark.gpu

PAD = 8                                               # elements kept beyond every capacity
ROWS = ("pk_idx", "pk_env", "pk_floor", "tags", "gap")
BIG_ND = 2 ** 62


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


def _batch(sr):
    return [(c, w) for c, w in zip(MC.cases(), MC.expected()) if c["sr"] == sr]


# ---- 1. tables made directly --------------------------------------------------------------- #
def _launch(det, sr, cases, cap=None, cap_ref=None, roff=None, env=True, window=MC.WINDOW):
    """bpmx_marks_device on mark tables uploaded directly, every output filled with 0xFF bytes first -> host
    arrays, the marks' offsets, the capacity."""
    import torch
    dev = det.device
    F = len(cases)
    if roff is None:
        roff = np.concatenate([[0], np.cumsum([len(c["ms"]) for c in cases])]).astype(np.int64)
    rtot = int(max(roff.max(), 0))
    cap_ref = rtot if cap_ref is None else cap_ref
    cap = (rtot | 1) if cap is None else cap              # odd
    rf_ms = np.concatenate([c["ms"] for c in cases] + [np.full(PAD, 1000, np.int32)]).astype(np.int32)
    rf_type = np.concatenate([c["type"] for c in cases] + [np.full(PAD, 1, np.int32)]).astype(np.int32)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    nd = None
    if any(c["nd"] is not None for c in cases):
        nd = up(np.array([BIG_ND if c["nd"] is None else c["nd"] for c in cases], np.int64))
    t = dict(roff=up(roff), rf_ms=up(rf_ms), rf_type=up(rf_type), nd=nd)
    ff = lambda n, dt: torch.full((n,), -1, dtype=dt, device=dev).view(torch.uint8).fill_(0xFF).view(dt)  # noqa: E731
    n = cap + PAD
    out = dict(pk_off=ff(F + 1 + PAD, torch.int64), pk_idx=ff(n, torch.int32), pk_env=ff(n, torch.float64),
               pk_floor=ff(n, torch.float64), tags=ff(n, torch.int8), gap=ff(n, torch.int32),
               final_idx=ff(n, torch.int32), bpm_t=ff(n, torch.float64), bpm=ff(n, torch.float64),
               n_final=ff(F + PAD, torch.int32), n_bpm=ff(F + PAD, torch.int32), status=ff(F + PAD, torch.int32),
               pass_=ff(3 * (F + PAD), torch.float64), record=ff((F + PAD) * N.MARKS_RECORD, torch.int32))
    k = N.PackedOut()
    k.cap_peaks, k.pk_off, k.pk_idx = cap, out["pk_off"].data_ptr(), out["pk_idx"].data_ptr()
    if env:
        k.pk_env, k.pk_floor = out["pk_env"].data_ptr(), out["pk_floor"].data_ptr()
    o = N.BeatsOut()
    for name in ("final_idx", "n_final", "bpm_t", "bpm", "n_bpm", "pass_", "tags", "status"):
        setattr(o, name, out[name].data_ptr())
    r = N.RefMarks(cap_ref, t["roff"].data_ptr(), t["rf_ms"].data_ptr(), t["rf_type"].data_ptr())
    mp = N.MarksParams(window)
    N.check(det.L.bpmx_marks_device(det.ctx, F, sr, ctypes.byref(mp), ctypes.byref(r),
                                    None if nd is None else nd.data_ptr(), ctypes.byref(k), ctypes.byref(o),
                                    out["gap"].data_ptr(), out["record"].data_ptr(), det.stream_handle()),
            "bpmx_marks_device")
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in out.items()}, roff, cap


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(raw, cases, want, roff, cap, cap_ref=None, env=True):
    """Every file against the host's rows and curve; everything no file owns against the 0xFF bytes."""
    F = len(cases)
    cap_ref = int(roff[-1]) if cap_ref is None else cap_ref
    counts = [len(w["idx"]) if 0 <= roff[f] <= roff[f + 1] <= cap_ref else 0 for f, w in enumerate(want)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert raw["pk_off"][:F + 1].tolist() == off.tolist()          # the true totals, whatever the capacity
    own = {k: np.zeros(len(raw[k]), bool) for k in ROWS + ("final_idx", "bpm_t", "bpm")}
    own_f = np.zeros(F + PAD, bool)
    seen = set()
    for f, (c, w) in enumerate(zip(cases, want)):
        st, a, n = int(raw["status"][f]), int(off[f]), counts[f]
        seen.add(st)
        if not (0 <= roff[f] <= roff[f + 1] <= cap_ref) or off[f + 1] > cap:
            assert st == N.MARKS_OVERFLOW, c["name"]
            continue
        own_f[f] = True
        nf, nb = int(raw["n_final"][f]), int(raw["n_bpm"][f])
        got = {"status": st, "record": raw["record"][f * N.MARKS_RECORD:(f + 1) * N.MARKS_RECORD],
               "idx": raw["pk_idx"][a:a + n], "tag": raw["tags"][a:a + n], "final": raw["final_idx"][a:a + nf],
               "bpm_t": raw["bpm_t"][a:a + nb], "bpm": raw["bpm"][a:a + nb]}
        MC.assert_same(got, w, c["name"])
        MC.check_identity(got["record"], len(c["ms"]))
        assert not raw["gap"][a:a + n].any() and np.isnan(raw["pass_"][3 * f:3 * f + 3]).all(), c["name"]
        for k in ROWS:
            own[k][a:a + n] = True
        if env:
            qnan = np.full(n, np.nan).view(np.uint64) if n else np.zeros(0, np.uint64)
            for k in ("pk_env", "pk_floor"):
                assert np.isnan(raw[k][a:a + n]).all() and (raw[k][a:a + n].view(np.uint64) >> 51 == qnan >> 51).all()
        own["final_idx"][a:a + nf] = True
        own["bpm_t"][a:a + nb] = own["bpm"][a:a + nb] = True
    if not env:
        own["pk_env"][:] = own["pk_floor"][:] = False
    for k, m in own.items():
        assert _untouched(raw[k][~m]), f"{k}: a write outside the files' used entries"
    for k in ("n_final", "n_bpm"):
        assert _untouched(raw[k][~own_f]), k
    assert _untouched(raw["status"][F:]) and _untouched(raw["pk_off"][F + 1:])
    assert _untouched(raw["record"].reshape(-1, N.MARKS_RECORD)[~own_f])
    assert _untouched(raw["pass_"].reshape(-1, 3)[~own_f])
    return seen


@pytest.mark.parametrize("sr", MC.RATES)
def test_ragged_batch_equals_the_host(det, sr):
    cases, want = zip(*_batch(sr))
    raw, roff, cap = _launch(det, sr, cases)
    assert cap % 2 == 1
    seen = _check(raw, cases, want, roff, cap)
    assert N.MARKS_OVERFLOW not in seen and N.OK in seen
    if sr == 147:
        st = {c["name"]: int(raw["status"][f]) for f, c in enumerate(cases)}
        assert [st[n] for n in ("n0", "one_s1", "one_s2", "same_sample", "only_s2", f"s1_{MC.LIMIT}",
                                f"s1_{MC.LIMIT + 8}")] == [N.MARKS_FEW] * 5 + [N.OK] * 2
        assert sum(int(o) % 2 for o in roff[:-1]) >= 3                  # slices at odd offsets


@pytest.mark.parametrize("sr", MC.RATES)
def test_both_workspace_routes_give_the_same(det, sr):
    cases, want = zip(*_batch(sr))
    plain, roff, cap = _launch(det, sr, cases)
    det.set_options(N.OPT_MARKS_GLOBAL)
    try:
        forced, _, _ = _launch(det, sr, cases)
    finally:
        det.set_options(0)
    _check(forced, cases, want, roff, cap)
    for k in plain:
        assert plain[k].tobytes() == forced[k].tobytes(), k


def test_without_env_and_floor_and_another_window(det):
    cases = [c for c in MC.cases() if c["sr"] == 1000]
    want = [MC.expect(c, 2.0) for c in cases]
    raw, roff, cap = _launch(det, 1000, cases, env=False, window=2.0)
    _check(raw, cases, want, roff, cap, env=False)
    assert any(len(w["bpm"]) and w["bpm"].tobytes() != e["bpm"].tobytes()
               for w, (c, e) in zip(want, _batch(1000)))                       # the window is read


def test_single_file_and_no_marks_at_all(det):
    (c, w), = [(c, w) for c, w in _batch(1000) if c["name"] == "window_edges"]
    raw, roff, cap = _launch(det, 1000, [c])
    _check(raw, [c], [w], roff, cap)
    empty = [c for c in MC.cases() if c["name"] == "n0"] * 3
    raw, roff, cap = _launch(det, 147, empty, cap=0)
    assert _check(raw, empty, [MC.expected()[0]] * 3, roff, 0) == {N.MARKS_FEW}


def test_capacity_below_the_total(det):
    cases, want = zip(*_batch(147))
    total = sum(len(w["idx"]) for w in want)
    for cap in (total - 1, total // 2, 1, 0):
        raw, roff, _ = _launch(det, 147, cases, cap=cap)
        seen = _check(raw, cases, want, roff, cap)                              # pk_off holds the true totals
        assert N.MARKS_OVERFLOW in seen and int(raw["pk_off"][len(cases)]) == total > cap
    # the marks' capacity one short: the last file's slice reaches past it, and it counts no rows
    raw, roff, cap = _launch(det, 147, cases, cap_ref=int(sum(len(c["ms"]) for c in cases)) - 1)
    _check(raw, cases, want, roff, cap, cap_ref=int(roff[-1]) - 1)
    assert raw["status"][len(cases) - 1] == N.MARKS_OVERFLOW and (raw["status"][:len(cases) - 1] != N.MARKS_OVERFLOW).all()


def test_descending_rf_off_gives_the_status_and_nothing_else(det):
    cases, want = zip(*_batch(1000))
    roff = np.concatenate([[0], np.cumsum([len(c["ms"]) for c in cases])]).astype(np.int64)
    bad = roff.copy()
    bad[2] = roff[1] - 1                                  # file 1 descends; file 2 then spans two files' marks
    bad[4] = -3                                           # file 3 ends, file 4 starts, before the table
    raw, _, cap = _launch(det, 1000, cases, roff=bad)
    F = len(cases)
    bad_files = {1, 3, 4}
    exp = list(want)
    rf_ms = np.concatenate([c["ms"] for c in cases])
    rf_ty = np.concatenate([c["type"] for c in cases])
    nd = [BIG_ND if c["nd"] is None else c["nd"] for c in cases]
    span = dict(name="span", sr=1000, nd=nd[2], ms=rf_ms[bad[2]:bad[3]], type=rf_ty[bad[2]:bad[3]])
    exp[2] = MC.expect(span)
    cs = list(cases)
    cs[2] = span
    for f in bad_files:
        assert raw["status"][f] == N.MARKS_OVERFLOW, f
    _check(raw, cs, exp, bad, cap, cap_ref=int(roff[-1]))
    assert set(np.flatnonzero(raw["status"][:F] == N.MARKS_OVERFLOW).tolist()) == bad_files


def test_to_host_raises_when_the_table_is_too_small(det):
    tables = [dict(ms=c["ms"], type=c["type"]) for c, _ in _batch(147)]
    total = sum(len(w["idx"]) for _, w in _batch(147))
    b = det.marks_device(tables, 147, MC.params(), cap_peaks=total - 1)
    with pytest.raises(N.BpmxError) as e:
        b.to_host()
    assert e.value.code == N.E_LIMIT
    res = det.marks_device(tables, 147, MC.params()).to_host()                 # the default capacity always suffices
    for (c, w), r in zip(_batch(147), res):
        assert r["raw_peaks"].tolist() == w["idx"].tolist() and r["marks_record"].tolist() == w["record"].tolist()
        assert r["final_peaks"].tolist() == w["final"].tolist() and r["bpm"].tobytes() == w["bpm"].tobytes(), c["name"]
        assert r["tags"].tolist() == w["tag"].tolist() and r["start_bpm"] != r["start_bpm"]


# ---- 2. the chain ------------------------------------------------------------------------- #
def _assert_metrics_same(got, want, where):
    """Two final_metrics dicts: the curve, and the device's normal form of both, bit for bit."""
    if want is None:
        assert got is None, where
        return
    assert got is not None, where
    assert TM.bits(got["bpm_times"]) == TM.bits(want["bpm_times"]), where
    assert TM.bits(got["smoothed_bpm"].values) == TM.bits(want["smoothed_bpm"].values), where
    assert np.array_equal(got["smoothed_bpm"].index.asi8, want["smoothed_bpm"].index.asi8), where
    M.assert_same(M.normal_form(got), M.normal_form(want), where, bits=True)


def _chain(det, tables, sr, params, gap_sec=5.0, nd=None):
    import torch
    with det.lock, torch.cuda.stream(det.host_stream()):
        b = det.marks_device(tables, sr, params, nd=nd)
        met = det.metrics_device(b, params).to_host()
        lab = det.labels_device(b, gap_sec).to_host()
        det.host_stream().synchronize()
    return met, lab


def _random_tables(n_files, seed):
    """Corrected label tables as tests/score_cases.py derives them from detected ones."""
    from tests import score_cases as SC
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_files):
        det_tab = SC.detected(int(rng.integers(2, 260)), seed * 100 + f)
        out.append(SC.corrected(det_tab, seed * 100 + 50 + f, spans=1 + f % 3))
    return out


@pytest.mark.parametrize("gap_sec", [3.0, 5.0])
def test_chain_equals_revise_on_random_tables(det, gap_sec):
    from tests import score_cases as SC
    tables = _random_tables(12, 5) + [LB.empty_table(), None]
    met, lab = _chain(det, tables, SC.SR, C.PARAMS, gap_sec)
    n = 0
    for f, t in enumerate(tables):
        want = LB.revise(t, SC.SR, C.PARAMS, gap_sec)
        r = met[f]
        assert r["marks_record"].tolist() == want["record"].tolist(), f
        assert r["raw_peaks"].tolist() == want["rows"]["idx"].tolist() and r["tags"].tolist() == want["rows"]["type"].tolist()
        assert r["final_peaks"].tolist() == (want["final_peaks"].tolist() if want["status"] == LB.MARKS_OK else []), f
        _assert_metrics_same(r["final_metrics"], want["final_metrics"], f)
        assert LB.same(lab[f], want["labels"]), f
        n += want["labels"] is not None and len(want["labels"]["pairs"]["dt"]) > 3
    assert n >= 8 and met[-1]["final_metrics"] is None and lab[-1] is None


def test_chain_equals_the_reference_made_goldens(det, tmp_path):
    from bpm_analysis_amd import beats as B
    from bpm_analysis_amd import reports as RP
    from tests import labels_cases as LC
    from tests import test_beats as TB
    by_key = {}
    for name in TM.NAMES:
        fx, params, table = TM.fixture(name)
        by_key.setdefault((int(fx["sr"]), bytes(N.metric_params(params)), params["output_smoothing_window_sec"]),
                          []).append((name, fx, params, table))
    for (sr, _, _), members in by_key.items():
        for gap in (1, 5.0):
            met, lab = _chain(det, [t for _, _, _, t in members], sr, members[0][2], gap)
            for (name, fx, params, table), r, lb in zip(members, met, lab):
                assert r["marks_record"].tolist() == fx["record"].tolist(), name
                assert r["final_peaks"].tolist() == fx["final_peaks"].tolist(), name
                m = r["final_metrics"]
                TM.assert_metrics(m, fx, name)
                fname = os.path.join(str(tmp_path), name + "_corrected.wav")
                assert TB._drop_stamp(RP.summary_text(fname, m)) == str(fx["summary_md"]), name
                p = tmp_path / f"{name}.csv"
                assert B.write_bpm_csv(str(p), m) and p.read_bytes().decode().replace("\r\n", "\n") == \
                    str(fx["csv"]).replace("\r\n", "\n"), name
                LC.assert_same(lb, LC.expected(fx, gap), (name, gap))
                if gap == 5.0:
                    assert LB.labels_csv_text(lb).encode("utf-8") == str(fx["text"]).encode("utf-8"), name


def _write(path, table):
    """A label file as a person's tool leaves it: the rows in the table's order."""
    with open(path, "w", encoding="utf-8") as f:
        f.write(LB.HEADER)
        for t, k in zip(table["time"].tolist(), table["type"].tolist()):
            if k in (LB.S1, LB.S2) and t == t:
                f.write(f"{t!r},60.0,{LB.TYPE_NAME[int(k)]}\n")


def test_score_label_files_equals_the_host(det, tmp_path):
    from bpm_analysis_amd import dropin as D
    from tests import score_cases as SC
    a, b = _random_tables(6, 7), _random_tables(6, 8)
    b[2] = a[2]                                           # two raters who agree
    pa, pb = [], []
    for k in range(6):
        pa.append(str(tmp_path / f"a{k}_labels.csv"))
        pb.append(str(tmp_path / f"b{k}_labels.csv"))
        _write(pa[-1], a[k])
        _write(pb[-1], b[k])
    pb[4] = str(tmp_path / "missing_labels.csv")
    got = D.score_label_files(pa, pb, SC.SR, tol_sec=SC.TOL_SEC, gap_sec=SC.GAP_SEC)
    assert isinstance(got[4]["error"], FileNotFoundError)
    for k in (0, 1, 2, 3, 5):
        first = LB.revise(LB.read_labels(pa[k]), SC.SR, C.PARAMS, SC.GAP_SEC)["labels"]
        want = LB.score(None if first is None else first["table"], LB.read_labels(pb[k]), SC.TOL_SEC, SC.GAP_SEC)
        assert got[k]["record"].tolist() == np.asarray(want["record"]).tolist() and got[k]["status"] == want["status"], k
        SC.check_identities(got[k]["record"], 0 if first is None else len(first["table"]["time"]))
    s = got[2]["record"]
    assert s[LB.SR_FP] == s[LB.SR_FN] == s[LB.SR_SWAP] == 0 and s[LB.SR_TP] > 10 and s[LB.SR_MAX_ABS] <= 2


# ---- 3. the closed loop ------------------------------------------------------------------- #
def test_closed_loop_from_the_analysis_own_labels(det):
    """The label tables of an analysis, read back as a person's marks, give the analysis' own beats, curve,
    metrics and label table."""
    from oracle import oracle as O
    fs = 44100
    recs = [O.synth(80 + i, n, fs, 1) for i, n in enumerate((fs * 20, fs * 20 + 7, fs * 17, fs * 20))]
    base = det.run_host_reports(recs, fs, C.PARAMS, labels=True, label_gap_sec=3.0)
    sr = int(base[0]["sr"])
    tables = [LB.parse_labels(LB.labels_csv_text(r["labels"])) for r in base]          # through the file's text
    met, lab = _chain(det, tables, sr, C.PARAMS, 3.0, nd=[int(r["n_env"]) for r in base])
    n = 0
    for f, (r, g, lb) in enumerate(zip(base, met, lab)):
        assert r["labels"] is not None and len(r["final_peaks"]) > 10, f
        assert g["final_peaks"].tolist() == r["final_peaks"].tolist(), f
        assert g["bpm"].tobytes() == r["bpm"].tobytes() and g["bpm_times"].tobytes() == r["bpm_times"].tobytes(), f
        rec = g["marks_record"].tolist()
        assert rec[3:] == [0] * 5 and rec[0] == len(r["labels"]["table"]["time"]) and rec[1] == len(r["final_peaks"])
        if r["metrics_source"] == "device":
            _assert_metrics_same(g["final_metrics"], r["final_metrics"], f)
            n += 1
        want = dict(r["labels"], table=dict(r["labels"]["table"], pos=np.arange(rec[0], dtype=np.int64)))
        assert LB.same(lb, want), f                       # the rows are the labelled peaks: positions count those
    assert n >= 3


# ---- 4. the drop-in entry point ----------------------------------------------------------- #
def test_revise_from_labels_end_to_end(det, tmp_path):
    from bpm_analysis_amd import dropin as D
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    names = TM.NAMES[:3]
    paths, rates, want = [], [], []
    for name in names:
        fx, params, table = TM.fixture(name)
        paths.append(str(src / f"{name}_labels.csv"))
        _write(paths[-1], table)
        rates.append(int(fx["sr"]))
        want.append(LB.revise(LB.read_labels(paths[-1]), rates[-1], C.PARAMS))
    paths.append(str(src / "nobody_labels.csv"))
    rates.append(302)
    got = D.revise_from_labels(paths, rates, C.PARAMS, str(out))
    assert isinstance(got[3]["error"], FileNotFoundError)
    files = ("_corrected_Analysis_Summary.md", "_corrected_bpm_plot.csv", "_corrected_labels.csv")
    assert sorted(os.listdir(str(out))) == sorted(n + s for n in names for s in files)
    for k, name in enumerate(names):
        g, w = got[k], want[k]
        assert g["sr"] == rates[k] and g["marks_record"].tolist() == w["record"].tolist(), name
        assert g["final_peaks"].tolist() == w["final_peaks"].tolist(), name
        _assert_metrics_same(g["final_metrics"], w["final_metrics"], name)
        assert LB.same(g["labels"], w["labels"]), name
        assert sorted(g["written"]) == sorted(str(out / (name + s)) for s in files) and g["skipped"] == []
        assert (out / f"{name}_corrected_labels.csv").read_bytes() == LB.labels_csv_text(w["labels"]).encode("utf-8")
        host_csv = tmp_path / "host.csv"
        from bpm_analysis_amd import beats as B
        assert B.write_bpm_csv(str(host_csv), w["final_metrics"])
        assert (out / f"{name}_corrected_bpm_plot.csv").read_bytes() == host_csv.read_bytes(), name
        assert (out / f"{name}_corrected_Analysis_Summary.md").read_text().startswith(
            f"# Analysis Report for: {name}_corrected\n"), name
    # nothing is overwritten unless asked
    hand = out / f"{names[0]}_corrected_labels.csv"
    hand.write_text("mine\n")
    again = D.revise_from_labels(paths[:1], rates[0], C.PARAMS, str(out))
    assert hand.read_text() == "mine\n" and again[0]["written"] == [] and len(again[0]["skipped"]) == 3
    again = D.revise_from_labels(paths[:1], rates[0], C.PARAMS, str(out), overwrite=True)
    assert hand.read_bytes() == LB.labels_csv_text(want[0]["labels"]).encode("utf-8") and len(again[0]["written"]) == 3
    # without a directory nothing is written
    D.revise_from_labels(paths[:1], rates[0], C.PARAMS)
    assert len(os.listdir(str(out))) == 9
