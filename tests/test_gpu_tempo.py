"""bpmx_tempo_device (k_tempo) on the MI355X against ``tempo.tempogram_ints`` at
the bounds of tests/tempo_cases.py: the CPU cases as batches, ragged batches at
several rates and lag ranges with sentinels around every output, a long
recording among short ones, the golden envelopes, and the drop-in route
(automatic start hints read on the device, ``_tempo.csv``).  Only one form of
the kernel exists (f64 VALU), so there is no second form to hold it against."""
import ctypes
import json
import os

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import tempo as TP
from tests import tempo_cases as TC

pytestmark = pytest.mark.gpu

PAD = 8                                               # elements kept beyond every output


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


def _run(det, envs, sr, ints, min_strength=0.3, start_windows=3):
    """The batch through bpmx_tempo_device into outputs pre-filled with 0xFF and PAD entries too long; returns
    ``Tempo.to_host``'s dicts after checking that nothing beyond the window total or the file count was written."""
    import torch
    from bpm_analysis_amd.engine import Tempo
    win, hop, kmin, kmax = ints
    fo = np.zeros(len(envs) + 1, np.int64)
    fo[1:] = np.cumsum([len(e) for e in envs])
    F, dev = len(envs), det.device
    res = det.alloc(fo, 1, sr)
    flat = np.concatenate([np.asarray(e, np.float64) for e in envs] + [np.zeros(0)])
    if len(flat):
        res.env[:len(flat)].copy_(torch.from_numpy(flat).to(dev))
    woff = np.zeros(F + 1, np.int64)
    woff[1:] = np.cumsum([TP.n_windows(len(e), win, hop) for e in envs])
    tot = int(woff[-1])
    assert [det.L.bpmx_tempo_windows(len(e), win, hop) for e in envs] == np.diff(woff).tolist()
    def full(n, dt):
        v = torch.empty(n + PAD, dtype=dt, device=dev)
        v.view(torch.uint8).fill_(0xFF)
        return v
    t = dict(lag=full(tot, torch.int32), rho=full(tot, torch.float64), bpm=full(tot, torch.float64),
             n_valid=full(F, torch.int32), n_strong=full(F, torch.int32), median_bpm=full(F, torch.float64),
             mean_rho=full(F, torch.float64), hint=full(F, torch.float64))
    p = N.TempoParams(win, hop, kmin, kmax, float(min_strength), int(start_windows), 0)
    i, o = N.Out(), N.TempoOut()
    i.env = res.env.data_ptr()
    for name, _ in N.TempoOut._fields_:
        setattr(o, name, t[name].data_ptr())
    with det.lock:
        N.check(det.L.bpmx_tempo_device(det.ctx, F, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, int(sr),
                                        ctypes.byref(p), ctypes.byref(i), ctypes.byref(o), det.stream_handle()),
                "bpmx_tempo_device")
    torch.cuda.synchronize()
    for name, v in t.items():
        n = tot if name in ("lag", "rho", "bpm") else F
        tail = v[n:].view(torch.uint8).cpu().numpy()
        assert len(tail) == PAD * v.element_size() and (tail == 0xFF).all(), name
    out = Tempo(det=det, sr=int(sr), win=win, hop=hop, kmin=kmin, kmax=kmax, min_strength=float(min_strength),
                start_windows=int(start_windows), woff=woff, lag=t["lag"][:tot], rho=t["rho"][:tot], bpm=t["bpm"][:tot],
                n_valid=t["n_valid"][:F], n_strong=t["n_strong"][:F], median_bpm=t["median_bpm"][:F],
                mean_rho=t["mean_rho"][:F], hint=t["hint"][:F])
    return out.to_host()


def _oracle(env, sr, ints, min_strength=0.3, start_windows=3):
    return TP.tempogram_ints(env, sr, *ints, min_strength=min_strength, start_windows=start_windows, detail=True)


def _check(got, envs, sr, ints, names, **kw):
    for g, e, name in zip(got, envs, names):
        want = _oracle(e, sr, ints, **kw)
        TC.check_inputs(dict(name=name, win=ints[0]), want)
        TC.assert_close(g, want, name)
        assert np.array_equal(g["time"], want["time"]), name


def test_cpu_cases_as_batches(det):
    """Every case of the core's CPU test, batched by its integers; the exact ones give the oracle's doubles."""
    groups = {}
    for c, w in zip(TC.cases(), TC.expected()):
        key = (c["sr"], c["win"], c["hop"], c["kmin"], c["kmax"], c["min_strength"], c["start_windows"])
        if not c["name"].startswith("golden_"):
            groups.setdefault(key, []).append((c, w))
    assert len(groups) >= 6
    for (sr, win, hop, kmin, kmax, ms, sw), members in groups.items():
        got = _run(det, [c["env"] for c, _ in members], sr, (win, hop, kmin, kmax), ms, sw)
        for g, (c, want) in zip(got, members):
            TC.assert_close(g, want, c["name"], exact=c["exact"])
            if c["exact"]:
                assert np.array_equal(g["rho"], want["rho"]) and np.array_equal(g["bpm"], want["bpm"]), c["name"]


def _envelope(rng, n, sr, bpm, special=None, win=0):
    """A smoothed positive random envelope with heart-rate pulses; `special` replaces its second window's span."""
    x = TC.smooth(rng, n, width=max(3, sr // 30), period=max(4, int(60 * sr / bpm)))
    if special is not None and n >= 2 * win:
        a = 2 * (win // 4)                               # window 2 of the tests' geometries (hop = win / 4) starts here
        if special == "constant":
            x[a:a + win] = 0.125
        elif special == "nan":
            x[a + 5] = np.nan
        elif special == "inf":
            x[a + 7], x[a + win // 2] = np.inf, -np.inf
        elif special == "ramp":
            x[:] = np.arange(n) * 0.001
    return x


GEOMETRIES = [
    ("sr302", 302, TP.geometry(302)),                                   # the usual rate: 380 lags, not a multiple of 16
    ("sr147", 147, TP.geometry(147)),
    ("sr1000", 1000, TP.geometry(1000)),
    ("sr302_30_300", 302, TP.geometry(302, dict(min_bpm=30, max_bpm=300))),
    ("sr147_win_odd", 147, (1179, 293, 38, 219)),                       # win not a multiple of 4
    ("sr1000_30_300", 1000, TP.geometry(1000, dict(min_bpm=30, max_bpm=300))),     # 135 KB of LDS per workgroup
]


@pytest.mark.parametrize("name,sr,ints", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_ragged_batch(det, name, sr, ints):
    win, hop, kmin, kmax = ints
    assert (kmin - 1) % 16 and (kmax + 2) % 16                          # the lag range ends on no multiple of 16
    rng = np.random.default_rng(sr + kmax)
    lens = [16, win - 1, win, win + 1, win + hop - 1, win + hop, 3 * win + 5, 18124]
    envs = [_envelope(rng, n, sr, 70 + 9 * k) for k, n in enumerate(lens)]
    for k, special in enumerate(("constant", "nan", "inf", "ramp")):
        envs.append(_envelope(rng, 2 * win + hop + 3 + k, sr, 95, special, win))
    offs = np.cumsum([len(e) for e in envs])
    assert (offs[:-1] % 2 == 1).sum() >= 3                              # slices start at odd offsets
    got = _run(det, envs, sr, ints)
    _check(got, envs, sr, ints, [f"{name}_{k}" for k in range(len(envs))])
    assert [len(g["lag"]) for g in got[:6]] == [0, 0, 1, 1, 1, 2]
    for g, special in zip(got[8:], ("constant", "nan", "inf", "ramp")):
        assert (g["lag"] == 0).any() and (special == "ramp" or (g["lag"] != 0).any()), special
    assert all(g["n_valid"] > 0 for g in got[2:8])


def test_long_recording_among_short_ones(det):
    sr, ints = 302, TP.geometry(302)
    rng = np.random.default_rng(11)
    lens = [3000, 200000, 16, 5000]
    envs = [_envelope(rng, n, sr, 60 + 25 * k) for k, n in enumerate(lens)]
    envs[1][:] = np.concatenate([_envelope(rng, 100000, sr, 64), _envelope(rng, 100000, sr, 131)])    # a median to find
    got = _run(det, envs, sr, ints, min_strength=0.4, start_windows=2)
    assert len(got[1]["lag"]) == 328 > 4 * 64 and 0 < got[1]["n_strong"] <= got[1]["n_valid"]
    _check(got, envs, sr, ints, [f"long_{k}" for k in range(4)], min_strength=0.4, start_windows=2)


def test_golden_envelopes(det):
    """The golden envelopes through ``Detector.alloc`` and ``tempo_device`` at the defaults; none of their decisions is open."""
    import torch
    names = ["vulpine", "nat_44k_60s_mono", "ref_44k_60s_mono", "ref_44k_10s_zeros"]
    envs = [TC.golden_env(n)[0] for n in names]
    assert {TC.golden_env(n)[1] for n in names} == {302}
    fo = np.zeros(len(envs) + 1, np.int64)
    fo[1:] = np.cumsum([len(e) for e in envs])
    with torch.cuda.stream(det.host_stream()):
        res = det.alloc(fo, 1, 302)
        res.env.copy_(torch.from_numpy(np.concatenate(envs)).to(det.device))
        tp = det.tempo_device(res)
        got = tp.to_host()
        det.host_stream().synchronize()
    assert (tp.win, tp.hop, tp.kmin, tp.kmax, tp.min_strength, tp.start_windows) == (2416, 604, 76, 453, 0.3, 3)
    for g, e, n in zip(got, envs, names):
        want = TP.tempogram(e, 302, detail=True)
        op, flat = TC.open_windows(want)
        assert not op.any() and not flat.any(), n
        TC.check_inputs(dict(name=n, win=2416), want)
        TC.assert_close(g, want, n, max_open=0.0)
        for k in ("sr", "win", "hop", "kmin", "kmax", "min_strength", "start_windows"):
            assert g[k] == want[k], k
    assert len(got[0]["lag"]) == 185 and np.array_equal(got[0]["lag"], np.loadtxt(os.path.join(TC.GOLDEN, "vulpine_tempo_lag.txt"), dtype=np.int32))
    assert got[3]["n_valid"] == 0 and np.isnan(got[3]["hint"])           # an all-zero envelope: NaN is "no hint"


def test_drop_in_auto_hints_and_tempo_csv(tmp_path):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin as D
    from tests import beats_cases as C
    from tests import test_beats as TB
    from tests import test_gpu_trace as GT
    from tests.golden import inputs as I
    src, auto_d, typed_d, plain_d = (tmp_path / n for n in ("src", "auto", "typed", "plain"))
    for p in (src, auto_d, typed_d, plain_d):
        p.mkdir()
    paths, pcms = [], []
    for k, spec in enumerate(GT.E2E):
        pcm, fs = I.make_input(spec)
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
        pcms.append((pcm, fs))
    params = dict(C.PARAMS, save_filtered_wav=False)
    auto = D.analyze_wav_files_to_reports(paths, params, str(auto_d), start_bpm_hints="auto", tempo=True)
    used = [r["start_bpm_hint"] for r in auto]
    assert any(h is not None for h in used)
    typed = D.analyze_wav_files_to_reports(paths, params, str(typed_d), start_bpm_hints=used)
    plain = D.analyze_wav_files_to_reports(paths, params, str(plain_d))
    bases = [os.path.basename(os.path.splitext(p)[0]) for p in paths]
    assert sorted(os.listdir(str(typed_d))) == sorted(b + s for b in bases for s in GT.SUFFIXES)
    assert sorted(os.listdir(str(plain_d))) == sorted(b + s for b in bases for s in GT.SUFFIXES)      # no _tempo.csv
    assert sorted(os.listdir(str(auto_d))) == sorted(b + s for b in bases for s in GT.SUFFIXES + ("_tempo.csv",))
    for k, base in enumerate(bases):
        a, t, p = auto[k], typed[k], plain[k]
        assert not {"tempo", "tempo_check", "start_bpm_hint"} & set(t) and not {"tempo", "tempo_check", "start_bpm_hint"} & set(p)
        # the hand-over on the device: the same beats and curve as from the downloaded hints as numbers
        assert np.array_equal(a["final_peaks"], t["final_peaks"]) and a["bpm"].tobytes() == t["bpm"].tobytes()
        assert a["bpm_times"].tobytes() == t["bpm_times"].tobytes()
        for sfx in GT.SUFFIXES:
            x, y = (auto_d / (base + sfx)).read_text(encoding="utf-8"), (typed_d / (base + sfx)).read_text(encoding="utf-8")
            if sfx.endswith(".md"):
                x, y = TB._drop_stamp(x), TB._drop_stamp(y)
            assert x == y, (base, sfx)
        assert json.loads((auto_d / (base + "_Analysis_Settings.json")).read_text())["start_bpm_hint"] == used[k]
        # the table is the oracle's on the envelope the run made
        pcm, fs = pcms[k]
        h = D.detect(pcm, fs, params)
        want = TP.tempogram(h["env"], h["sr"], params, detail=True)
        TC.check_inputs(dict(name=base, win=want["win"]), want)
        TC.assert_close(a["tempo"], want, base)
        assert used[k] == (None if np.isnan(want["hint"]) else a["tempo"]["hint"])
        assert a["tempo_check"] == TP.compare(a["tempo"], a["bpm_times"], a["bpm"])
        got, chk = TP.read_csv(str(auto_d / (base + "_tempo.csv")))
        TC.assert_close(got, want, base + "_csv")
        assert chk == a["tempo_check"] and np.array_equal(got["bpm"], a["tempo"]["bpm"], equal_nan=True)
        ref = str(tmp_path / "oracle_tempo.csv")
        TP.write_csv(ref, want)
        assert open(ref).readline() == open(str(auto_d / (base + "_tempo.csv"))).readline()
        assert len(TP.read_csv(ref)[0]["lag"]) == len(got["lag"]) > 0
