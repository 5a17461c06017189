"""bpmx_hrvspec_device (k_hrvspec) on the MI355X against
``hrv_spectrum.spectrum_ints`` at the derived bound of tests/hrvspec_cases.py:
the CPU cases as batches, a ragged batch at three rates with a long recording
among short ones and sentinels around every output, the optional q, both forms
of the kernel, a table too small for the last file, and the Python routes
(``run_host_reports``, the drop-in with ``_hrv_spectrum.csv``, corrected marks,
the lengths that marks beats need)."""
import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import hrv_spectrum as HS
from tests import hrvspec_cases as HC

pytestmark = pytest.mark.gpu

PAD = 8                                               # entries kept beyond every output
PER_WINDOW = ("code", "n_rr", "lf_peak", "hf_peak", "t_mid", "var", "lf", "hf")


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


def _run(det, files, sr, g, want_q=True, cap=None, extra=(1, 0, 3), raw=False):
    """`files`: (final beats, nd, beats status) per recording, through bpmx_hrvspec_device into outputs pre-filled
    with 0xFF and PAD entries too long.  The beats lie in a table whose slices are `extra` entries longer than the
    beats, so they start at odd offsets.  Returns ``HrvSpectrum.to_host``'s dicts (`raw`: the arrays as they are)
    after checking that nothing beyond the window total or the file count was written."""
    import torch
    from bpm_analysis_amd.engine import HrvSpectrum
    F, dev = len(files), det.device
    pk_off = np.zeros(F + 1, np.int64)
    pk_off[1:] = np.cumsum([len(i) + extra[f % len(extra)] for f, (i, _, _) in enumerate(files)])
    total = int(pk_off[-1])
    cap = total if cap is None else cap
    fin = np.full(max(total, 1), -7, np.int32)
    for f, (i, _, _) in enumerate(files):
        fin[pk_off[f]:pk_off[f] + len(i)] = i
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_off, d_fin = up(pk_off), up(fin[:max(cap, 1)])
    d_nf, d_st = up(np.array([len(i) for i, _, _ in files], np.int32)), up(np.array([s for _, _, s in files], np.int32))
    lengths = np.array([nd for _, nd, _ in files], np.int64)
    fo = np.zeros(F + 1, np.int64)
    fo[1:] = np.cumsum(lengths)
    woff = np.zeros(F + 1, np.int64)
    woff[1:] = np.cumsum([HS.n_windows(int(n), g["win"], g["hop"]) for n in lengths])
    tot, nq = int(woff[-1]), g["n_freq"]
    assert [det.L.bpmx_hrvspec_windows(int(n), g["win"], g["hop"]) for n in lengths] == np.diff(woff).tolist()

    def full(n, dt):
        v = torch.empty(n + PAD, dtype=dt, device=dev)
        v.view(torch.uint8).fill_(0xFF)
        return v
    t = {k: full(tot, torch.int32 if k in ("code", "n_rr", "lf_peak", "hf_peak") else torch.float64) for k in PER_WINDOW}
    t["q"] = full(tot * nq, torch.float64) if want_q else None
    t["record"], t["status"] = full(F * N.HRVSPEC_RECORD, torch.float64), full(F, torch.int32)
    k, b, o = N.PackedOut(), N.BeatsOut(), N.HrvspecOut()
    k.cap_peaks, k.pk_off = cap, d_off.data_ptr()
    b.final_idx, b.n_final, b.status = d_fin.data_ptr(), d_nf.data_ptr(), d_st.data_ptr()
    for name, _ in N.HrvspecOut._fields_:
        setattr(o, name, None if t[name] is None else t[name].data_ptr())
    p = N.hrvspec_params(g)
    with det.lock:
        N.check(det.L.bpmx_hrvspec_device(det.ctx, F, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, int(sr),
                                          ctypes.byref(p), ctypes.byref(k), ctypes.byref(b), ctypes.byref(o),
                                          det.stream_handle()), "bpmx_hrvspec_device")
    torch.cuda.synchronize()
    used = dict({k_: tot for k_ in PER_WINDOW}, q=tot * nq, record=F * N.HRVSPEC_RECORD, status=F)
    for name, v in t.items():
        if v is None:
            continue
        tail = v[used[name]:].view(torch.uint8).cpu().numpy()
        assert len(tail) == PAD * v.element_size() and (tail == 0xFF).all(), name
    if raw:
        return {k_: (None if v is None else v[:used[k_]].cpu().numpy()) for k_, v in t.items()}, woff
    out = HrvSpectrum(det=det, beats=None, sr=int(sr), g=dict(g), lengths=lengths, woff=woff,
                      **{k_: (None if v is None else v[:max(used[k_], 1)]) for k_, v in t.items()})
    return out.to_host()


def _oracle(idx, nd, sr, g, st=0):
    return HS.spectrum_ints(idx, nd, sr, g, beats_ok=st == 0, detail=True)


def test_cpu_cases_as_batches(det):
    """Every case of the core's CPU test, batched by its integers."""
    groups = {}
    for c, w in zip(HC.cases(), HC.expected()):
        key = (c["sr"],) + tuple(c["g"][k] for k in HS.INT_KEYS + HS.FLOAT_KEYS)
        groups.setdefault(key, []).append((c, w))
    assert len(groups) >= 10
    used = 0.0
    for members in groups.values():
        c0 = members[0][0]
        got = _run(det, [(c["idx"], c["nd"], 0 if c["ok"] else -2) for c, _ in members], c0["sr"], c0["g"])
        for g_, (c, want) in zip(got, members):
            assert HC.open_peaks(want) == [], c["name"]
            used = max(used, HC.assert_close(g_, want, c["name"]))
    print(f"largest share of the bound on q used: {used:.2e}")


def _ragged(sr):
    """Recordings of 0, 1 and 2 windows, one of about 3,000 beats and more than 64 windows, short ones around it."""
    g = HS.geometry(sr)
    win, hop = g["win"], g["hop"]
    long_ = HC.rhythm(3000, sr, sr=sr, base=0.72, depth=0.05)
    files = [(HC.rhythm(40, 1, sr=sr), 0, 0), (HC.rhythm(150, 2, sr=sr), win - 5, 0),
             (HC.rhythm(260, 3, sr=sr), win + hop, 0), (long_, int(long_[-1]) + 11, 0),
             (HC.rhythm(170, 4, sr=sr), win + 1, 0), (HC.rhythm(3, 5, sr=sr), win, 0),
             (HC.rhythm(200, 6, sr=sr), win + hop - 1, -2)]
    return g, files


@pytest.mark.parametrize("sr", [302, 147, 1000])
def test_ragged_batch(det, sr):
    g, files = _ragged(sr)
    got = _run(det, files, sr, g, extra=(1, 3, 0, 5))
    assert [len(r["code"]) for r in got[:3]] == [0, 1, 2] and len(got[3]["code"]) > 64 and len(files[3][0]) > 3000
    for f, (r, (idx, nd, st)) in enumerate(zip(got, files)):
        want = _oracle(idx, nd, sr, g, st)
        assert HC.open_peaks(want) == [], (sr, f)
        HC.assert_close(r, want, f"ragged_{sr}_{f}")
    assert got[3]["record"][0] > 64 and got[6]["status"] == N.HRVSPEC_NONE and got[5]["status"] == N.HRVSPEC_OK


def test_q_set_and_null_give_the_same_bands(det):
    g, files = _ragged(147)
    a, woff = _run(det, files, 147, g, want_q=True, raw=True)
    b, _ = _run(det, files, 147, g, want_q=False, raw=True)
    assert b["q"] is None and a["q"] is not None and len(a["q"]) == int(woff[-1]) * g["n_freq"]
    for k in PER_WINDOW + ("record", "status"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_both_forms_against_the_oracle(det):
    """The rotation along the grid (default) and one sincos per term (BPMX_OPT_HRVSPEC_DIRECT)."""
    c = [x for x in HC.cases() if x["name"] in ("wander1", "golden_vulpine")]
    want = [w for x, w in zip(HC.cases(), HC.expected()) if x["name"] in ("wander1", "golden_vulpine")]
    assert c[0]["g"] == c[1]["g"] and c[0]["sr"] == c[1]["sr"] == 302
    files = [(x["idx"], x["nd"], 0) for x in c]
    try:
        det.set_options(N.OPT_HRVSPEC_DIRECT)
        direct = _run(det, files, 302, c[0]["g"])
    finally:
        det.set_options(0)
    rot = _run(det, files, 302, c[0]["g"])
    for d, r, w, x in zip(direct, rot, want, c):
        ud, ur = HC.assert_close(d, w, x["name"] + "_direct"), HC.assert_close(r, w, x["name"] + "_rotate")
        print(f"{x['name']}: share of the bound on q used: direct {ud:.2e}, rotate {ur:.2e}")
        assert np.array_equal(d["code"], r["code"]) and np.array_equal(d["lf_peak"], r["lf_peak"])
    assert not np.array_equal(direct[0]["q"], rot[0]["q"])              # two forms, not one


def test_overflow_leaves_the_file_alone(det):
    g, files = _ragged(147)
    files = files[:5]
    total = sum(len(i) + e for (i, _, _), e in zip(files, (1, 0, 3, 1, 0)))
    raw, woff = _run(det, files, 147, g, cap=total - 1, raw=True)
    full, _ = _run(det, files, 147, g, raw=True)
    assert raw["status"].tolist() == [0, 0, 0, 0, N.HRVSPEC_OVERFLOW]
    a, b = int(woff[4]), int(woff[5])
    assert b > a
    for k in PER_WINDOW:                                                # nothing of the last file was written
        assert (raw[k][a:b].view(np.uint8) == 0xFF).all(), k
        assert raw[k][:a].tobytes() == full[k][:a].tobytes(), k         # the other files are intact
    assert (raw["q"][a * g["n_freq"]:].view(np.uint8) == 0xFF).all()
    assert (raw["record"][4 * N.HRVSPEC_RECORD:].view(np.uint8) == 0xFF).all()
    assert raw["record"][:4 * N.HRVSPEC_RECORD].tobytes() == full["record"][:4 * N.HRVSPEC_RECORD].tobytes()


def _e2e_inputs():
    from tests import test_gpu_trace as GT
    from tests.golden import inputs as I
    return [I.make_input(spec) for spec in GT.E2E]


def test_run_host_reports_carries_the_spectrum(det):
    from tests import beats_cases as C
    params = dict(C.PARAMS, save_filtered_wav=False)
    ins = _e2e_inputs()
    groups = {}
    for pcm, fs in ins:                                       # a batch is one rate, format and channel count
        groups.setdefault((fs, pcm.dtype.str, pcm.ndim), []).append(pcm)
    n = 0
    for (fs, _, _), pcms in groups.items():
        got = det.run_host_reports(pcms, fs, params, hrv_spectrum=True)
        plain = det.run_host_reports(pcms, fs, params)
        for r, p in zip(got, plain):
            assert "hrv_spectrum" in r and "hrv_spectrum" not in p and set(r) - set(p) == {"hrv_spectrum"}
            want = HS.spectrum(r["final_peaks"], r["n_env"], r["sr"], params, detail=True)
            assert HC.open_peaks(want) == [], n
            HC.assert_close(r["hrv_spectrum"], want, f"e2e_{n}")
            for key in HS.INT_KEYS + HS.FLOAT_KEYS + ("sr",):
                assert r["hrv_spectrum"][key] == want[key], key
            assert len(r["hrv_spectrum"]["code"]) == 1 and r["hrv_spectrum"]["n_rr"][0] > 0
            assert np.array_equal(r["final_peaks"], p["final_peaks"]) and r["bpm"].tobytes() == p["bpm"].tobytes()
            n += 1
    assert n == len(ins)


def test_drop_in_writes_the_csv(tmp_path):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin as D
    from tests import beats_cases as C
    from tests import test_beats as TB
    from tests import test_gpu_trace as GT
    src, with_d, plain_d = (tmp_path / n for n in ("src", "with", "plain"))
    for p in (src, with_d, plain_d):
        p.mkdir()
    paths = []
    for k, (pcm, fs) in enumerate(_e2e_inputs()):
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
    params = dict(C.PARAMS, save_filtered_wav=False)
    res = D.analyze_wav_files_to_reports(paths, params, str(with_d), hrv_spectrum=True)
    plain = D.analyze_wav_files_to_reports(paths, params, str(plain_d))
    bases = [os.path.basename(os.path.splitext(p)[0]) for p in paths]
    assert sorted(os.listdir(str(plain_d))) == sorted(b + s for b in bases for s in GT.SUFFIXES)   # no such file
    assert sorted(os.listdir(str(with_d))) == sorted(b + s for b in bases for s in GT.SUFFIXES + ("_hrv_spectrum.csv",))
    for k, base in enumerate(bases):
        assert "hrv_spectrum" in res[k] and "hrv_spectrum" not in plain[k]
        for sfx in GT.SUFFIXES:                               # the reports are today's, apart from the time stamps
            x, y = (with_d / (base + sfx)).read_text(encoding="utf-8"), (plain_d / (base + sfx)).read_text(encoding="utf-8")
            if sfx.endswith(".md"):
                x, y = TB._drop_stamp(x), TB._drop_stamp(y)
            assert x == y, (base, sfx)
        d, got = res[k]["hrv_spectrum"], HS.read_csv(str(with_d / (base + "_hrv_spectrum.csv")))
        want = HS.spectrum(res[k]["final_peaks"], res[k]["n_env"], res[k]["sr"], params, detail=True)
        HC.assert_close(d, want, base)
        assert np.array_equal(got["lf"], d["lf"], equal_nan=True) and np.array_equal(got["hf"], d["hf"], equal_nan=True)
        assert np.array_equal(got["code"], d["code"]) and np.array_equal(got["record"], d["record"], equal_nan=True)
        assert len(got["code"]) == HS.n_windows(res[k]["n_env"], d["win"], d["hop"]) >= 1


def _mark_tables():
    from bpm_analysis_amd import labels as LB
    out = []
    for seed, n in ((1, 400), (2, 30), (3, 0)):
        ms = np.round(HC.rhythm(n, seed, sr=1000) * 1.0).astype(np.int64)          # beat times in ms
        out.append(dict(ms=ms.astype(np.int32), type=np.full(len(ms), LB.S1, np.int32)))
    return out


def test_marks_route_equals_the_oracle_on_the_corrected_beats(det):
    import torch
    from tests import beats_cases as C
    params = dict(C.PARAMS, save_filtered_wav=False)
    tables, sr = _mark_tables(), 147
    lengths = [(int(t["ms"][-1]) * sr + 500) // 1000 + 1 for t in tables]
    with det.lock, torch.cuda.stream(det.host_stream()):
        b = det.marks_device(tables, sr, params)
        hs = det.hrv_spectrum_device(b, lengths=lengths, params=params, want_q=True)
        beats, got = b.to_host(), hs.to_host()
        det.host_stream().synchronize()
    assert len(got[0]["code"]) > 5 and (got[0]["code"] == 0).any()
    for f, (r, bt, n) in enumerate(zip(got, beats, lengths)):
        fin = bt["final_peaks"]
        want = HS.spectrum(fin, n, sr, params, detail=True)
        if len(fin) < 2:
            want["status"] = HS.NONE                                     # BPMX_MARKS_FEW is a beats status that is not OK
        assert HC.open_peaks(want) == [], f
        HC.assert_close(r, want, f"marks_{f}")
    assert got[2]["status"] == N.HRVSPEC_NONE


def test_marks_beats_need_lengths(det):
    from tests import beats_cases as C
    params = dict(C.PARAMS, save_filtered_wav=False)
    b = det.marks_device(_mark_tables(), 147, params)
    with pytest.raises(ValueError, match="lengths"):
        det.hrv_spectrum_device(b, params=params)
    with pytest.raises(ValueError, match="one entry per recording"):
        det.hrv_spectrum_device(b, lengths=[1000], params=params)
