"""Rectified mode on the GPU: the labeler's envelope of filtered WAVs
(heartbeat_labeler.py:53-67) and the detection stages on it.

Expected envelopes come from the pandas call the labeler makes
(tests/rect_cases.py recipe) and are compared as uint64 patterns (NaN positions
where the result is NaN).  Shapes are the smallest that cross a boundary of the
kernels: T is the chunk of outputs a workgroup takes, L the prefix entries the
LDS variant holds."""
import dataclasses
import os

import numpy as np
import pytest

from tests import goldens as G
from tests import rect_cases as C

pytestmark = pytest.mark.gpu

K = C.plan_constants()
T, L = K["RECT_CHUNK"], K["RECT_LDS_N"]
FS_SMALL = (10, 20, 30, 300, 302, 310, 320)            # w = 1, 2, 3, 30, 30, 31, 32
FS_OVER_T = (T + 1) * 10                               # w = T + 1: a window longer than a chunk, still in LDS
FS_OVER_LDS = (L - T + 1) * 10                         # w one past the LDS variant: the global-prefix variant
PAD = 32                                               # 0xFF words kept past the total


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


@pytest.fixture(scope="module")
def params():
    return dict(G.BASE_PARAMS)


def _seed(test, name, ch):
    return 1000 * test + 10 * list(C.DTYPES).index(name) + ch


def _lengths(w):
    """The ragged batch of the issue, an empty recording among them; ordered so
    that slices start at odd offsets."""
    off = (w - 1) // 2
    lens = [T + 1, 2, 1, w - 1, w, w + 1, 0, T - 1, T, 2 * T + off + 1]
    lens = [n for n in lens if n >= 0]
    starts = np.cumsum([0] + lens[:-1])
    assert sum(int(s) % 2 for s in starts) >= 3
    return lens


def _envelope(det, recs, fs, params, options=0, byte_off=0, stages=None):
    """ENVELOPE stage of a rectified run over host recordings -> (env words with
    the PAD tail, Result).  The PCM lies `byte_off` bytes past an aligned base;
    env is pre-filled with 0xFF."""
    import torch
    from bpm_analysis_amd import _native as N
    ch = 1 if recs[0].ndim == 1 else recs[0].shape[1]
    flat = np.concatenate([np.ascontiguousarray(r).reshape(-1) for r in recs])
    raw = torch.zeros(byte_off + flat.nbytes + 64, dtype=torch.uint8, device=det.device)
    raw[byte_off:byte_off + flat.nbytes] = torch.from_numpy(flat.view(np.uint8).copy()).to(det.device)
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
           np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[flat.dtype]
    pcm = raw[byte_off:byte_off + flat.nbytes].view(tdt)
    assert pcm.data_ptr() % 16 == byte_off % 16
    fo = np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])]).astype(np.int64)
    out = det.alloc(fo, 1, fs)
    tot = int(fo[-1])
    out.env = torch.full((tot + PAD,), -1, dtype=torch.int64, device=det.device).view(torch.float64)
    det.run(pcm, fo, fs, params, mode="rectified", stages=N.STAGE_ENVELOPE if stages is None else stages,
            channels=ch, out=out, options=options)
    torch.cuda.synchronize()
    return out.env.cpu().numpy(), out


def _check_envelope(words, recs, w, what):
    fo = np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])])
    assert (words[fo[-1]:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all(), what
    for f, r in enumerate(recs):
        assert C.same_bits(words[fo[f]:fo[f + 1]], C.recipe(r, w)), (what, f, r.shape)


def _batches(rng, name, ch, w):
    ragged = [C.make(rng, name, n, ch) for n in _lengths(w)]
    single = [C.make(rng, name, 2 * T + (w - 1) // 2 + 1, ch)]
    return ragged, single


@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("name", C.INT_NAMES)
def test_envelope_integer_route(det, params, name, ch):
    from bpm_analysis_amd import _native as N
    rng = np.random.default_rng(_seed(1, name, ch))
    for fs in FS_SMALL + (FS_OVER_T,):
        w = fs // 10
        for recs in _batches(rng, name, ch, w):
            words, _ = _envelope(det, recs, fs, params)
            _check_envelope(words, recs, w, (name, ch, fs, len(recs)))
            seq, _ = _envelope(det, recs, fs, params, options=N.OPT_RECT_SEQ)
            assert seq.tobytes() == words.tobytes(), (name, ch, fs, "OPT_RECT_SEQ")


@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("name", C.INT_NAMES)
def test_envelope_window_beyond_the_lds_variant(det, params, name, ch):
    from bpm_analysis_amd import _native as N
    rng = np.random.default_rng(_seed(2, name, ch))
    w = FS_OVER_LDS // 10
    assert w + T > L
    single = [C.make(rng, name, int(1.3 * w), ch)]
    ragged = [C.make(rng, name, n, ch) for n in _lengths(w)]
    for recs in (single, ragged):
        words, _ = _envelope(det, recs, FS_OVER_LDS, params)
        _check_envelope(words, recs, w, (name, ch, len(recs)))
        seq, _ = _envelope(det, recs, FS_OVER_LDS, params, options=N.OPT_RECT_SEQ)
        assert seq.tobytes() == words.tobytes()


@pytest.mark.parametrize("name,ch,byte_off", [("i16", 1, 2), ("u8", 1, 1), ("u8", 2, 1), ("i16", 2, 2), ("i16", 1, 0)])
def test_envelope_unaligned_pcm_base(det, params, name, ch, byte_off):
    """2 bytes off for int16 mono (the run realigns the base and moves the frame
    offsets), 1 byte off for u8; int16 stereo 2 bytes off puts its frames across
    the 16-byte vectors."""
    rng = np.random.default_rng(99 + byte_off + ch)
    for fs in (302, 320, FS_OVER_LDS):
        w = fs // 10
        recs = [C.make(rng, name, n, ch) for n in _lengths(w)]
        words, _ = _envelope(det, recs, fs, params, byte_off=byte_off)
        _check_envelope(words, recs, w, (name, ch, byte_off, fs))


def test_empty_recording_is_flagged_and_its_neighbours_are_whole(det, params):
    from bpm_analysis_amd import _native as N
    rng = np.random.default_rng(5)
    recs = [C.make(rng, "i16", n, 1) for n in (7, 0, 9)]
    words, out = _envelope(det, recs, 302, params)
    _check_envelope(words, recs, 30, "empty")
    flags = out.flags.cpu().numpy()
    assert flags[1] & N.F_TOO_SHORT and not flags[0] & N.F_TOO_SHORT and not flags[2] & N.F_TOO_SHORT


@pytest.mark.parametrize("name,ch", [("f32", 1), ("f32", 2), ("f64", 1), ("f64", 2), ("i16", 3)])
def test_envelope_general_route(det, params, name, ch):
    rng = np.random.default_rng(_seed(3, name, ch))
    for fs in FS_SMALL + (FS_OVER_T,):
        w = fs // 10
        for recs in _batches(rng, name, ch, w):
            words, _ = _envelope(det, recs, fs, params)
            _check_envelope(words, recs, w, (name, ch, fs, len(recs)))


def test_bad_arguments_write_nothing(det, params, monkeypatch):
    import torch
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd import engine
    rng = np.random.default_rng(3)
    rec = C.make(rng, "i16", 500, 1)
    pcm = torch.from_numpy(rec).to(det.device)
    fo = np.array([0, 500], dtype=np.int64)

    def attempt(fs, d=None, want_y=False, stages=N.STAGE_ALL):
        out = det.alloc(fo, 1 if d is None else d.ds, fs, want_y=want_y)
        for t in (out.env, out.floor, out.troughs, out.peaks):
            t.view(torch.int64).fill_(-1)
        for t in (out.flags, out.n_troughs, out.n_peaks):
            t.fill_(-7)
        with pytest.raises(N.BpmxArgError):
            det.run(pcm, fo, fs, params, mode="rectified", out=out, d=d, stages=stages)
        torch.cuda.synchronize()
        for t in (out.env, out.floor, out.troughs, out.peaks):
            assert bool((t.view(torch.int64) == -1).all())
        for t in (out.flags, out.n_troughs, out.n_peaks):
            assert bool((t == -7).all())

    attempt(302, d=dataclasses.replace(engine.detect_design(302, params), ds=2))
    attempt(9, stages=N.STAGE_ENVELOPE)                            # env_window 0
    with pytest.raises(N.BpmxArgError):                            # the Python layer refuses y
        det.run(pcm, fo, 302, params, mode="rectified", want_y=True)
    monkeypatch.setattr(engine, "_no_filtered_signal", lambda *a: None)
    attempt(302, want_y=True)                                      # and so does the library: out.y set


@pytest.fixture(scope="module")
def vulpine():
    g = G.load("vulpine")
    assert g["pcm"].dtype == np.int16 and int(g["fs"]) == 302
    return g, C.recipe(g["pcm"], 30)


def _same_detection(r, e):
    for k in ("floor", "troughs", "peaks"):
        assert np.array_equal(np.asarray(r[k]), np.asarray(e[k]), equal_nan=True), k
    assert r["n_raw_troughs"] == e["n_raw_troughs"] and r["flags"] == e["flags"]


def test_known_answer_from_raw_samples(det, vulpine):
    from bpm_analysis_amd import _native as N
    g, env = vulpine
    r = det.run_host([g["pcm"]], 302, g["params"], mode="rectified")[0]
    assert r["sr"] == 302 and C.same_bits(r["env"], env)
    e = det.run_env_host([env], 302, g["params"], N.STAGE_FLOOR | N.STAGE_PEAKS)[0]
    _same_detection(r, e)
    assert len(g["log_peaks"]) == 1456 and np.array_equal(r["peaks"], g["log_peaks"])
    assert r["flags"] & N.F_TROUGH_TIE
    rs = det.run_host([g["pcm"]], 302, g["params"], mode="rectified", resolve_ties=True)[0]
    es = det.run_env_host([env], 302, g["params"], N.STAGE_FLOOR | N.STAGE_PEAKS, resolve_ties=True)[0]
    assert C.same_bits(rs["env"], env)
    _same_detection(rs, es)
    assert rs["flags"] & N.F_TROUGH_ORDERED and not rs["flags"] & N.F_TROUGH_TIE
    assert np.array_equal(rs["peaks"], g["log_peaks"])


def test_pipeline_setting_falls_back_to_one_run(det, vulpine):
    """bpmx_set_pipeline does not apply to the mode: same results with it set."""
    g, _ = vulpine
    recs = [np.ascontiguousarray(g["pcm"][1000 * k:1000 * k + 20000 + 101 * k]) for k in range(4)]
    want = det.run_host(recs, 302, g["params"], mode="rectified")
    det.set_pipeline(2)
    try:
        got = det.run_host(recs, 302, g["params"], mode="rectified")
    finally:
        det.set_pipeline(0)
    for r, e, rec in zip(got, want, recs):
        assert C.same_bits(r["env"], C.recipe(rec, 30)) and C.same_bits(r["env"], e["env"])
        _same_detection(r, e)


def test_round_trip_through_the_debug_samples(det, params):
    """Reference mode's int16 debug samples fed back in rectified mode."""
    from bpm_analysis_amd import _native as N
    from oracle import oracle as O
    fs = 44100
    recs = [O.synth(40 + f, n, fs, 1) for f, n in enumerate((fs * 20, fs * 20 + 777, fs * 20 - 1234))]
    ref = det.run_host_y16(recs, fs, params, mode="reference")
    sr = ref[0]["sr"]
    y16 = [np.ascontiguousarray(r["y16"]) for r in ref]
    assert sr == 302 and all(y.dtype == np.int16 and len(y) > 6000 for y in y16)
    got = det.run_host(y16, sr, params, mode="rectified")
    envs = [C.recipe(y, sr // 10) for y in y16]
    want = det.run_env_host(envs, sr, params, N.STAGE_FLOOR | N.STAGE_PEAKS)
    for r, env, e in zip(got, envs, want):
        assert C.same_bits(r["env"], env)
        _same_detection(r, e)
        assert len(r["peaks"]) > 10


@pytest.fixture()
def wavs(tmp_path, vulpine):
    from scipy.io import wavfile
    g, _ = vulpine
    mono = np.ascontiguousarray(g["pcm"])
    stereo = np.stack([mono, np.roll(mono, 3) // 2], axis=1).astype(np.int16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [str(src / "a_filtered_debug.wav"), str(src / "b_stereo.wav")]
    wavfile.write(paths[0], 302, mono)
    wavfile.write(paths[1], 302, stereo)
    return g, paths, [mono, stereo]


def test_dropin_labeler_envelope_and_preprocess(det, wavs, tmp_path, monkeypatch):
    from bpm_analysis_amd import DEFAULT_PARAMS, dropin
    from bpm_analysis_amd.engine import Detector
    g, paths, audio = wavs
    for p, a in zip(paths, audio):
        env, sr = dropin.labeler_envelope(p)
        assert sr == 302 and C.same_bits(env, C.recipe(a, 30))
    outdir = tmp_path / "out"
    outdir.mkdir()
    before = sorted(os.listdir(os.path.dirname(paths[0])))
    prm = dict(DEFAULT_PARAMS, **g["params"])
    prm.update(bpmx_mode="rectified", save_filtered_wav=True, downsample_factor=300)
    env, sr = dropin.preprocess_audio(paths[0], prm, str(outdir))
    assert sr == 302 and C.same_bits(env, C.recipe(audio[0], 30))
    assert os.listdir(str(outdir)) == [] and sorted(os.listdir(os.path.dirname(paths[0]))) == before
    calls = []
    orig = Detector.run_env_host
    monkeypatch.setattr(Detector, "run_env_host", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    floor, troughs = dropin._calculate_dynamic_noise_floor(env, sr, prm)
    peaks = dropin.find_raw_peaks(env, sr, prm, floor.values)
    assert calls == []
    from bpm_analysis_amd import _native as N
    e = orig(det, [env], 302, prm, N.STAGE_FLOOR | N.STAGE_PEAKS, resolve_ties=True)[0]
    assert np.array_equal(floor.values, e["floor"], equal_nan=True) and np.array_equal(troughs, e["troughs"])
    assert np.array_equal(peaks, e["peaks"]) and np.array_equal(peaks, g["log_peaks"])


def test_dropin_batch_entry_points(det, wavs, tmp_path):
    from bpm_analysis_amd import DEFAULT_PARAMS, dropin
    from bpm_analysis_amd import _native as N
    g, paths, audio = wavs
    outdir = tmp_path / "out"
    outdir.mkdir()
    prm = dict(DEFAULT_PARAMS, **g["params"])
    prm["save_filtered_wav"] = False
    res = dropin.analyze_wav_files(paths, prm, str(outdir), mode="rectified")
    for r, a in zip(res, audio):
        assert "error" not in r
        env = C.recipe(a, 30)
        e = det.run_env_host([env], 302, prm, N.STAGE_FLOOR | N.STAGE_PEAKS, resolve_ties=True)[0]
        assert r["sr"] == 302 and C.same_bits(r["env"], env)
        for k in ("floor", "troughs", "peaks"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(e[k]), equal_nan=True), k
        assert r["flags"] == e["flags"]
    one = dropin.detect(audio[0], 302, prm, mode="rectified")
    assert C.same_bits(one["env"], res[0]["env"]) and np.array_equal(one["peaks"], res[0]["peaks"])
    rep = dropin.analyze_wav_files_to_reports(paths[:1], dict(prm, save_filtered_wav=True), str(outdir),
                                              mode="rectified")
    assert "error" not in rep[0] and rep[0]["final_metrics"] is not None
    base = os.path.splitext(os.path.basename(paths[0]))[0]
    made = sorted(os.listdir(str(outdir)))
    assert made == sorted(base + s for s in ("_bpm_plot.csv", "_Analysis_Summary.md", "_Debug_Log.md",
                                             "_Analysis_Settings.json"))
    with pytest.raises(N.BpmxArgError):
        det.run_host_y16([audio[0]], 302, prm, mode="rectified")
