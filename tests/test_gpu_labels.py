"""bpmx_labels_device (k_labels) on the MI355X: the beat goldens through
beats_device(trace=True) and labels_device against the fixtures the reference
labeler's functions made; tables made directly (tags, gap labels, final beats,
curve) against labels.py with sentinels around every output; both workspace
routes; the drop-in route's ``_labels.csv`` against the host route's.
Integers are compared for equality, doubles as bit patterns."""
import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from bpm_analysis_amd import labels as LB
from tests import beats_cases as C
from tests import labels_cases as LC
from tests import test_gpu_beats as G

pytestmark = pytest.mark.gpu

PAD = 8                                               # elements kept beyond every capacity
ROWS = LC.DEV_KEYS_I + LC.DEV_KEYS_F
OWNER = {k: {"lb": "n_labels", "pr": "n_pairs", "gr": "n_groups"}[k[:2]] for k in ROWS}


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


# ---- 1. the fixtures through the device -------------------------------------------------- #
def test_goldens_through_beats_and_labels(det):
    """The parity test: packed peak table -> beats_device(trace=True) -> labels_device equals what the
    labeler's functions gave for the reference's own strings, so the tags + gap rule is the rule on the strings."""
    import torch
    fx = {n: f for n, f, _ in LC.golden_cases()}
    groups = {}
    for name, g, t in C.golden_tables():
        groups.setdefault((bytes(H.beat_params(t["params"])), t["hint"], t["sr"]), []).append((name, t))
    n_ok = n_none = 0
    for members in groups.values():
        tables = [t for _, t in members]
        pk = G._upload(det, tables)
        b = det.beats_device(pk, tables[0]["params"], tables[0]["hint"], trace=True)
        labs = {gap: det.labels_device(b, gap) for gap in LC.GAPS}
        got = {gap: lab.to_host() for gap, lab in labs.items()}
        torch.cuda.synchronize()
        for f, (name, _) in enumerate(members):
            for gap in LC.GAPS:
                want = LC.expected(fx[name], gap)
                LC.assert_same(got[gap][f], want, (name, gap))
                n_ok += want is not None
                n_none += want is None
            if got[5.0][f] is not None:
                assert LB.labels_csv_text(got[5.0][f]) == str(fx[name]["text"]), name
    assert n_ok == 3 * 26 and n_none == 3 * 2


# ---- 2. tables made directly --------------------------------------------------------------- #
def _case(n_labels, seed, extra=3, kind="mixed", nan="none", gap_override=False, status=0):
    """A recording with `n_labels` labelled peaks among `extra` unlabelled ones."""
    rng = np.random.default_rng(seed)
    n = n_labels + extra
    raw = np.cumsum(rng.integers(30, 200, n)).astype(np.int64)
    types = np.zeros(n, np.int8)
    lab = np.sort(rng.choice(n, n_labels, replace=False))
    if kind == "mixed":
        types[lab] = np.where(np.arange(n_labels) % 2 == 0, 1, 2)
    elif kind == "s1":
        types[lab] = 1
    else:
        types[lab] = 2
    tags = np.where(types == 2, 2, np.where(types == 1, 1, 4)).astype(np.int8)
    gap = np.zeros(n, np.int32)
    if gap_override:
        s2 = np.flatnonzero(types == 2)
        tags[s2[::2]] = 4                             # Noise by the main pass, S2 by the last gap-fill pass
        gap[s2[::2]] = (N.TR_GAP_S1 << 0) | (N.TR_GAP_S2 << 8)
        no = np.flatnonzero(types == 0)
        tags[no] = 2                                  # S2 by the main pass, S1 by a gap-fill pass but not a final beat
        gap[no] = N.TR_GAP_S1 << 4
    fin = raw[types == 1]
    m = max(len(fin) - 1, 0)
    bt = fin[1:].astype(np.float64) / 302 if m else np.zeros(0)
    bv = rng.uniform(45, 190, m)
    if nan == "some" and m > 4:
        bv[[0, 1, m // 2]] = np.nan
    if nan == "all":
        bv[:] = np.nan
    return dict(raw=raw, tags=tags, gap=gap, strings=None, fin=fin, bt=bt, bv=bv, sr=302, status=status, types=types)


def _batch():
    return [("l0", dict(_case(0, 1, extra=0))), ("l1", _case(1, 2, kind="s1")), ("no_s2", _case(2, 3, kind="s1", extra=5)),
            ("l63", _case(63, 4, extra=2)), ("nan_rows", _case(64, 5, nan="some")),
            ("gap_override", _case(65, 6, extra=6, gap_override=True)), ("no_s1", _case(9, 7, kind="s2", extra=2)),
            ("nan_only", _case(31, 8, nan="all")), ("l129", _case(129, 9, extra=4))]


def _launch(det, cases, gap_sec, cap=None):
    """bpmx_labels_device on tables uploaded directly, every output filled with 0xFF bytes first -> host arrays."""
    import torch
    dev = det.device
    cnt = [len(c["raw"]) for c in cases]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    tot, F = int(off[-1]), len(cases)
    cap = tot if cap is None else cap
    size = max(tot, 1) + PAD

    def slices(key, dt, count):
        a = np.zeros(size, dt)
        for f, c in enumerate(cases):
            v = np.asarray(c[key]).astype(dt)[:count(c)]
            a[off[f]:off[f] + len(v)] = v
        return torch.from_numpy(a).to(dev)

    n_of = lambda c: len(c["raw"])  # noqa: E731
    t_idx, t_tags, t_gap = slices("raw", np.int32, n_of), slices("tags", np.int8, n_of), slices("gap", np.int32, n_of)
    t_fin = slices("fin", np.int32, lambda c: len(c["fin"]))
    t_bt, t_bv = slices("bt", np.float64, lambda c: len(c["bt"])), slices("bv", np.float64, lambda c: len(c["bv"]))
    per = lambda fn, dt: torch.from_numpy(np.array([fn(c) for c in cases], dt)).to(dev)  # noqa: E731
    t_nf, t_nb = per(lambda c: len(c["fin"]), np.int32), per(lambda c: len(c["bt"]), np.int32)
    t_st, t_off = per(lambda c: c["status"], np.int32), torch.from_numpy(off).to(dev)
    ones = lambda n, dt: torch.full((n,), -1, dtype=torch.int64 if dt == torch.float64 else dt,  # noqa: E731
                                    device=dev).view(dt)
    out = {k: ones(size, torch.float64 if k in LC.DEV_KEYS_F else torch.int32) for k in ROWS}
    out.update(n_labels=ones(F + PAD, torch.int32), n_pairs=ones(F + PAD, torch.int32),
               n_groups=ones(F + PAD, torch.int32), record=ones((F + PAD) * N.LABELS_RECORD, torch.float64),
               status=ones(F + PAD, torch.int32))
    k = N.PackedOut()
    k.cap_peaks, k.pk_off, k.pk_idx = cap, t_off.data_ptr(), t_idx.data_ptr()
    b = N.BeatsOut()
    b.final_idx, b.n_final, b.bpm_t, b.bpm = t_fin.data_ptr(), t_nf.data_ptr(), t_bt.data_ptr(), t_bv.data_ptr()
    b.n_bpm, b.tags, b.status = t_nb.data_ptr(), t_tags.data_ptr(), t_st.data_ptr()
    o = N.LabelsOut()
    for name, _ in N.LabelsOut._fields_:
        setattr(o, name, out[name].data_ptr())
    lp = N.LabelParams(float(gap_sec))
    N.check(det.L.bpmx_labels_device(det.ctx, F, 302, ctypes.byref(lp), ctypes.byref(k), ctypes.byref(b),
                                     t_gap.data_ptr(), ctypes.byref(o), det.stream_handle()), "bpmx_labels_device")
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in out.items()}, off


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(raw, off, cases, gap_sec, cap=None):
    """Every file against labels.py; everything no file owns against the sentinel."""
    F = len(cases)
    cap = int(off[-1]) if cap is None else cap
    owned = {k: np.zeros(len(raw[k]), bool) for k in ROWS}
    seen = set()
    for f, c in enumerate(cases):
        a, n = int(off[f]), len(c["raw"])
        st = int(raw["status"][f])
        seen.add(st)
        if a + n > cap:
            assert st == N.LABELS_OVERFLOW, f
            assert all(_untouched(raw[k][f:f + 1]) for k in ("n_labels", "n_pairs", "n_groups")), f
            assert _untouched(raw["record"][f * N.LABELS_RECORD:(f + 1) * N.LABELS_RECORD]), f
            continue
        cnt = {k: int(raw[k][f]) for k in ("n_labels", "n_pairs", "n_groups")}
        assert all(0 <= v <= n for v in cnt.values()), (f, cnt)
        dev = {k: raw[k][a:a + cnt[OWNER[k]]] for k in ROWS}
        dev["status"], dev["record"] = st, raw["record"][f * N.LABELS_RECORD:(f + 1) * N.LABELS_RECORD]
        LC.assert_same(LC.labels_of(dev, gap_sec), LC.host(c, gap_sec), (f, gap_sec))
        for k in ROWS:
            owned[k][a:a + cnt[OWNER[k]]] = True
    for k in ROWS:
        assert _untouched(raw[k][~owned[k]]), f"{k}: a write outside the files' used entries"
    for k in ("n_labels", "n_pairs", "n_groups", "status"):
        assert _untouched(raw[k][F:]), k
    assert _untouched(raw["record"][F * N.LABELS_RECORD:])
    return seen


@pytest.mark.parametrize("gap", [1, 5.0])
def test_direct_tables_ragged_batch(det, gap):
    named = _batch()
    cases = [c for _, c in named]
    assert [len(c["raw"]) % 2 for c in cases].count(1) >= 3            # slices at odd offsets
    raw, off = _launch(det, cases, gap)
    assert _check(raw, off, cases, gap) == {N.LABELS_OK, N.LABELS_NONE}
    by = {n: int(raw["n_labels"][f]) for f, (n, _) in enumerate(named)}
    assert (by["l0"], by["l1"], by["no_s2"], by["l63"], by["nan_rows"], by["gap_override"], by["l129"]) == \
        (0, 0, 2, 63, 64, 65, 129)
    st = {n: int(raw["status"][f]) for f, (n, _) in enumerate(named)}
    assert st["l0"] == st["l1"] == st["no_s1"] == st["nan_only"] == N.LABELS_NONE
    assert all(st[n] == N.LABELS_OK for n in ("no_s2", "l63", "nan_rows", "gap_override", "l129"))
    f = [n for n, _ in named].index("no_s2")
    assert int(raw["n_pairs"][f]) == 0 and int(raw["n_groups"][f]) == 0


def test_single_file(det):
    c = _case(129, 9, extra=4)
    raw, off = _launch(det, [c], 5.0)
    assert _check(raw, off, [c], 5.0) == {N.LABELS_OK} and int(raw["n_labels"][0]) == 129


@pytest.mark.parametrize("status", [N.BEATS_SKIPPED, H.E_FEW_PEAKS, N.BEATS_OVERFLOW])
def test_unfinished_beats_make_no_labels(det, status):
    cases = [c for _, c in _batch()]
    for f in (3, 5, 8):
        cases[f] = dict(cases[f], status=status)
    raw, off = _launch(det, cases, 5.0)
    _check(raw, off, cases, 5.0)
    assert [int(raw["status"][f]) for f in (3, 5, 8)] == [N.LABELS_NONE] * 3 and int(raw["status"][4]) == N.LABELS_OK


def test_capacity_one_short(det):
    cases = [c for _, c in _batch()]
    tot = sum(len(c["raw"]) for c in cases)
    raw, off = _launch(det, cases, 5.0, cap=tot - 1)
    seen = _check(raw, off, cases, 5.0, cap=tot - 1)
    assert N.LABELS_OVERFLOW in seen and int(raw["status"][len(cases) - 1]) == N.LABELS_OVERFLOW
    assert all(_untouched(raw[k][tot - 1:]) for k in ROWS)


def test_both_workspace_routes_give_the_same(det):
    cases = [c for _, c in _batch()] + [_case(701, 12, extra=9, nan="some")]     # one beyond the LDS limit
    plain, off = _launch(det, cases, 1)
    _check(plain, off, cases, 1)
    det.set_options(N.OPT_LABELS_GLOBAL)
    try:
        forced, _ = _launch(det, cases, 1)
    finally:
        det.set_options(0)
    for k in plain:
        assert plain[k].tobytes() == forced[k].tobytes(), k
    assert int(plain["n_labels"][len(cases) - 1]) == 701


# ---- 3. end to end ------------------------------------------------------------------------- #
E2E = [dict(seed=31, secs=9, fs=44100), dict(seed=32, secs=8, fs=44100, channels=2),
       dict(seed=33, secs=12, fs=44100, transform="clicks")]
SUFFIXES = ("_bpm_plot.csv", "_Analysis_Summary.md", "_Debug_Log.md", "_Analysis_Settings.json")


def _host_route(D, paths, params, outdir, mode):
    res = D.analyze_wav_files(paths, dict(params, save_filtered_wav=False), outdir, mode=mode)
    out = []
    for r in res:
        assert "error" not in r
        a = B.analyze_recording(r["env"], r["sr"], r["floor"], r["troughs"], r["peaks"], params, None)
        out.append(LB.from_analysis(a, r["sr"], 3.0))
    return out


@pytest.mark.parametrize("mode", ["reference", "rectified"])
def test_labels_file_equals_the_host_route(tmp_path, mode):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin as D
    from tests import test_beats as TB
    from tests.golden import inputs as I
    src, new, old, host = tmp_path / "src", tmp_path / "new", tmp_path / "old", tmp_path / "host"
    for p in (src, new, old, host):
        p.mkdir()
    paths = []
    for k, spec in enumerate(E2E):
        pcm, fs = I.make_input(spec)
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
    params = dict(C.PARAMS, save_filtered_wav=False)
    if mode == "rectified":                           # the labeler's input: the filtered debug WAVs of a reference run
        D.analyze_wav_files(paths, dict(params, save_filtered_wav=True), str(old), mode="reference")
        paths = [f"{os.path.splitext(p)[0]}_filtered_debug.wav" for p in paths]
        assert all(os.path.exists(p) for p in paths)
        for p in old.iterdir():
            p.unlink()
    plain = D.analyze_wav_files_to_reports(paths, params, str(old), mode=mode)
    got = D.analyze_wav_files_to_reports(paths, params, str(new), mode=mode, labels=True, label_gap_sec=3.0)
    want = _host_route(D, paths, params, str(host), mode)
    bases = [os.path.basename(os.path.splitext(p)[0]) for p in paths]
    assert sorted(os.listdir(str(old))) == sorted(b + s for b in bases for s in SUFFIXES)
    assert sorted(os.listdir(str(new))) == sorted(b + s for b in bases for s in SUFFIXES + ("_labels.csv",))
    for k, base in enumerate(bases):
        a, b = plain[k], got[k]
        assert "labels" not in a and "labels_written" not in a
        assert sorted(b) == sorted(list(a) + ["labels", "labels_written"]) and b["labels_written"] is True
        for key, v in a.items():                      # with labels=False every dict and file is what it was
            if isinstance(v, np.ndarray):
                assert v.tobytes() == b[key].tobytes(), key
            elif isinstance(v, (int, float, str, type(None))):
                assert v == b[key] or (v != v and b[key] != b[key]), key
        for sfx in SUFFIXES:
            x, y = (old / (base + sfx)).read_text(encoding="utf-8"), (new / (base + sfx)).read_text(encoding="utf-8")
            if sfx.endswith(".md"):
                x, y = TB._drop_stamp(x), TB._drop_stamp(y)
            assert x == y, (base, sfx)
        assert want[k] is not None and len(want[k]["pairs"]["dt"]) > 3
        LC.assert_same(b["labels"], want[k], base)
        hp = str(host / f"{base}_labels.csv")
        assert LB.write_labels(hp, want[k]) is True
        assert (new / f"{base}_labels.csv").read_bytes() == open(hp, "rb").read(), base
    # the file is where hand labels live: a second run leaves it alone unless told otherwise
    hand = str(new / f"{bases[0]}_labels.csv")
    with open(hand, "w") as f:
        f.write(LB.HEADER + "1.0,70.0,S1\n")
    again = D.analyze_wav_files_to_reports(paths[:1], params, str(new), mode=mode, labels=True, label_gap_sec=3.0)
    assert again[0]["labels_written"] is False and open(hand).read() == LB.HEADER + "1.0,70.0,S1\n"
    again = D.analyze_wav_files_to_reports(paths[:1], params, str(new), mode=mode, labels=True, label_gap_sec=3.0,
                                           labels_overwrite=True)
    assert again[0]["labels_written"] is True and open(hand, "rb").read() == \
        open(str(host / f"{bases[0]}_labels.csv"), "rb").read()
