"""Packed 24-bit PCM (BPMX_DT_I24) on the GPU: the format in every mode, and
native mode's matrix-core routes k_native_blocks_mfma24<3> / <5>.

An I24 batch means the BPMX_DT_I32 batch of the samples v << 8, so the
reference is the oracle on the expanded int32 samples, and wherever the I24
run takes the same arithmetic as the int32 run (reference mode, rectified
mode, native mode's generic kernel) the two are bit-identical.

Cases are tests/test_native_plan24.py's P24_CASES, shaped like
tests/test_gpu_native_formats.py's: fs = 320 ds and the recordings of
case_lengths (15 blocks; m bt, m bt + 1 and (m + 1) bt - 1 blocks; 1499
blocks; an inactive one of nd = 15), the samples of
native_cases.recording("i32", ...) & -256 packed to 3 bytes, plus one recording
of uniform noise over the full 24-bit range (the others' body is at half
scale, and the top plane needs its extremes).  ds 95, 96, 146 and 159 mono run
on the new routes, 160 mono and 146 stereo on the generic kernel's I24
instantiation.  A batch lies behind GUARD + off guard bytes for off in 0, 1, 2,
3 and 15 and before GUARD more, so the recordings' first bytes hit every
residue mod 4 and several mod 16 (asserted on the host).

Conditions on the inputs (CPU): the wrap-around discrimination of the existing
module, D >= 1e-3 per recording (these recordings give D >= 2), and every
value of both lower byte planes occurs in each case.

Per active recording, native mode: max |y - y_o| <= 1e-9 max |y_o| and the
same for env (TOL); the new routes agree with the BPMX_OPT_NATIVE_F64 run of
the same batch within 1e-12 of scale (TOL_F64); the generic I24 runs (ds 160,
stereo, and every case with BPMX_OPT_NATIVE_F64) are bit-identical to the
BPMX_DT_I32 run of the expanded samples in y, env, floor, troughs, peaks and
flags; detection equals the oracle's env-level functions on the GPU's own
envelope; the run without y is bit-identical; the outputs do not depend on the
batch's byte offset; the inactive recording has no outputs.  The largest
errors per route are recorded (record_property); DESIGN.md §8j lists what an
MI355X gave."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import native_cases as NC
from tests.test_gpu_hilbert_lengths import _oracle_answer
from tests.test_gpu_native_formats import (D_INT, GUARD, TOL_F64, _assert_inactive, _assert_same_runs,
                                           _check_against_oracle)
from tests.test_gpu_native_formats import _batch as _batch16
from tests.test_gpu_native_formats import _run as _run_arrays
from tests.test_gpu_params import _check, _same
from tests.test_native_plan import CASES, OPT_NATIVE_F64, case_lengths
from tests.test_native_plan24 import OFFSETS, P24, P24_CASES

SEED0 = 2400
ALL = ("y", "env", "floor", "troughs", "peaks")


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


def _noise(ch, n, seed):
    """Uniform over the full 24-bit range, both extremes present, as int32 v << 8."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-2 ** 23, 2 ** 23, (n, ch))
    v[n // 2], v[n // 2 + 1] = 2 ** 23 - 1, -2 ** 23
    v[0], v[-1] = 2 ** 23 - 1 - rng.integers(0, 2 ** 17, ch), -2 ** 23 + rng.integers(0, 2 ** 17, ch)
    x = (v * 256).astype(np.int32)
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


def _pack(x):
    """int32 samples with zero low bytes -> their 3 upper bytes, as they lie in a WAV file."""
    assert x.dtype == np.int32 and not np.any(x & 255)
    return np.ascontiguousarray(x.reshape(-1).astype("<i4").view(np.uint8).reshape(-1, 4)[:, 1:]).reshape(-1)


_batches = {}


def _batch(c):
    """A case's expanded recordings, their bytes and the oracle's answers, made once per module."""
    if c.name not in _batches:
        fs, p = NC.rate(c.ds), NC.params(c.ds)
        d = O.derive(fs, p)
        assert (d.ds, d.sr, d.env_w) == (c.ds, 320, 32)
        lens = case_lengths(c)
        recs = [NC.recording("i32", c.ch, n, fs, SEED0 + i) & np.int32(-256) for i, n in enumerate(lens[:5])]
        recs.append(_noise(c.ch, (2 * c.bt + 3) * c.ds + 5, SEED0 + 9))
        recs.append(NC.recording("i32", c.ch, lens[5], fs, SEED0 + 5) & np.int32(-256))
        ref = []
        for x in recs[:-1]:
            env, y = O.preprocess_native(x, d, return_y=True)
            x0 = x if c.ch == 1 else np.ascontiguousarray(x[:, 0])
            y0 = y if c.ch == 1 else O.preprocess_native(x0, d, return_y=True)[1]
            ref.append(dict(env=env, y=y, y_cast=NC.cast_y(x, d), d0=NC.discrimination(y0, NC.cast_y(x0, d))))
        assert -(-recs[-1].shape[0] // c.ds) == 15
        assert max(r.shape[0] for r in recs) * 3 < 1 << 20     # under 1 MB per channel: the batches stay small
        _batches[c.name] = dict(fs=fs, params=p, d=d, recs=recs, ref=ref, bytes=[_pack(r) for r in recs])
    return _batches[c.name]


def _run24(det, c, packed, lens, fs, params, off=0, want_y=True, opt=0, mode="native"):
    """The packed batch behind GUARD + off guard bytes and before GUARD more."""
    import torch
    flat = np.concatenate([np.full(GUARD + off, 0x7F, np.uint8)] + list(packed) + [np.full(GUARD, 0x7F, np.uint8)])
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = torch.from_numpy(flat).to(det.device)
    assert dev.data_ptr() % 16 == 0
    pcm = dev[GUARD + off:GUARD + off + 3 * int(fo[-1]) * c.ch]
    res = det.run(pcm, fo, fs, params, mode=mode, channels=c.ch, want_y=want_y, options=opt, sample_format="i24")
    torch.cuda.synchronize()
    out = res.to_host()
    del dev
    return out


def _run_case(det, c, b, **kw):
    return _run24(det, c, b["bytes"], [r.shape[0] for r in b["recs"]], b["fs"], b["params"], **kw)


def _run32(det, c, b, **kw):
    return _run_arrays(det, c._replace(dtype="i32", off=0), b["recs"], b["fs"], b["params"], **kw)


def test_inputs_discriminate_and_cover():
    """CPU conditions: D >= 1e-3 per recording (channel 0 for stereo, whose
    mean does not wrap), all 256 values of both lower planes and both extremes
    of the top plane in every case, and the first bytes' residues."""
    for c in P24_CASES:
        b = _batch(c)
        for k, r in enumerate(b["ref"]):
            print(f"{c.name} recording {k}: D = {r['d0']:.3f}")
            assert r["d0"] >= D_INT, (c.name, k, r["d0"])
            if c.ch > 1:
                assert np.array_equal(r["y"], r["y_cast"])
        by = np.concatenate(b["bytes"]).reshape(-1, 3)
        assert len(np.unique(by[:, 0])) == 256 and len(np.unique(by[:, 1])) == 256
        assert {0x7F, 0x80} <= set(np.unique(by[:, 2]).tolist())
        fo = np.concatenate([[0], np.cumsum([r.shape[0] for r in b["recs"]])])[:-1]
        first = {(GUARD + off + 3 * c.ch * int(f)) % 16 for off in OFFSETS for f in fo}
        assert {a % 4 for a in first} == {0, 1, 2, 3} and len(first) >= 8, (c.name, sorted(first))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in P24_CASES])
def test_native_case(det, record_property, name):
    c = P24[name]
    b = _batch(c)
    new_route = c.route.startswith("mfma24")
    worst = {"y": 0.0, "env": 0.0}
    with_y = _run_case(det, c, b)
    _check_against_oracle(c, b, with_y, worst)
    record_property(f"max_rel_err_y[{c.route}]", worst["y"])
    record_property(f"max_rel_err_env[{c.route}]", worst["env"])
    # any byte offset: the same bits
    for off in OFFSETS[1:]:
        _assert_same_runs(_run_case(det, c, b, off=off), with_y, (name, off), keys=ALL)
    plain = _run_case(det, c, b, off=3, want_y=False)
    _assert_same_runs(plain, with_y, name)
    for k, r in enumerate(plain[:-1]):
        _check(r, _oracle_answer(np.ascontiguousarray(r["env"]), b["params"], b["fs"]), (name, k))
    # the int32 run of the expanded samples, and the generic kernel on request
    i32 = _run32(det, c, b)
    f64 = _run_case(det, c, b, off=1, opt=OPT_NATIVE_F64)
    _assert_same_runs(f64, i32, (name, "f64 / i32"), keys=ALL)
    _assert_inactive(f64[-1], name)
    if new_route:
        for k, (x, y) in enumerate(zip(with_y[:-1], f64[:-1])):
            sy, se = np.max(np.abs(y["y"])), np.max(np.abs(y["env"]))
            ey, ee = np.max(np.abs(x["y"] - y["y"])) / sy, np.max(np.abs(x["env"] - y["env"])) / se
            print(f"{name} recording {k}: against the f64 kernel y {ey:.3e} env {ee:.3e}")
            assert ey <= TOL_F64 and ee <= TOL_F64, (name, k, ey, ee)
    else:
        _assert_same_runs(with_y, i32, (name, "i24 / i32"), keys=ALL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["i24x1/146", "i24x2/146"])
def test_reference_and_rectified_modes(det, name):
    """Reference mode: bit-identical to the int32 run and to the oracle's
    bit-exact path; rectified mode (ds = 1): bit-identical to the int32 run,
    on the exact-integer route and on the pandas recursion."""
    from bpm_analysis_amd import _native as N
    c = P24[name]
    b = _batch(c)
    import torch
    keep = [0, 1, 5, 6]                                        # 15 blocks, 2 bt blocks, the noise, the inactive one
    recs = [b["recs"][k] for k in keep]

    def run32(recs, mode, fs, params, opt=0):
        flat = np.concatenate([r.reshape(-1) for r in recs])
        fo = np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])]).astype(np.int64)
        res = det.run(torch.from_numpy(flat).to(det.device), fo, fs, params, mode=mode, channels=c.ch, options=opt)
        torch.cuda.synchronize()
        return res.to_host()

    def run24(recs, mode, fs, params, off, opt=0):
        return _run24(det, c, [_pack(r) for r in recs], [r.shape[0] for r in recs], fs, params, off=off, want_y=False,
                      opt=opt, mode=mode)
    want = run32(recs, "reference", b["fs"], b["params"])
    for off in (0, 1, 2, 3):
        got = run24(recs, "reference", b["fs"], b["params"], off)
        _assert_same_runs(got, want, (name, "reference", off))
        if off == 0:
            for k, x in enumerate(recs[:-1]):
                o = O.detect(x, b["fs"], b["params"])
                assert np.array_equal(got[k]["env"], o["env"]), (name, k)
                assert np.array_equal(got[k]["floor"], o["floor"], equal_nan=True), (name, k)
                assert np.array_equal(got[k]["troughs"], o["troughs"]) and np.array_equal(got[k]["peaks"], o["peaks"])
            _assert_inactive(got[-1], name)
    # rectified: the samples as they are at 320 Hz (window 32); the noise recording holds int32's most negative value
    mid = recs[2].shape[0] // 2
    short = [recs[0][:2000], recs[1][:2001], recs[2][mid - 1000:mid + 1000]]
    assert np.any(short[2] == np.iinfo(np.int32).min)
    for opt in (0, N.OPT_RECT_SEQ):
        want = run32(short, "rectified", 320, b["params"], opt)
        for off in (0, 1, 2, 3, 15):
            _assert_same_runs(run24(short, "rectified", 320, b["params"], off, opt), want, (name, "rectified", opt, off))


@pytest.mark.gpu
def test_recordings_do_not_leak_into_each_other(det):
    """Dropping any recording of the batch leaves the others' outputs bit-identical."""
    c = P24["i24x1/146"]
    b = _batch(c)
    lens = [r.shape[0] for r in b["recs"]]
    full = _run_case(det, c, b)
    for drop in range(len(lens)):
        keep = [k for k in range(len(lens)) if k != drop]
        part = _run24(det, c, [b["bytes"][k] for k in keep], [lens[k] for k in keep], b["fs"], b["params"], off=drop % 4)
        _assert_same_runs(part, [full[k] for k in keep], ("drop", drop), keys=ALL)


@pytest.mark.gpu
def test_tables_are_not_shared_with_int16():
    """ds = 95: the int16 and the 24-bit matrix-core routes have the same ds
    and bt, and tables that differ (key16).  Back to back in both orders on a
    fresh context each: the same bits as alone."""
    from bpm_analysis_amd.engine import Detector
    c24, c16 = P24["i24x1/95"], CASES["i16x1/95"]
    assert (c24.ds, c24.bt) == (c16.ds, c16.bt)
    b24, b16 = _batch(c24), _batch16(c16)
    runs = {}
    for order in ("24-16", "16-24"):
        d2 = Detector(0)
        for which in order.split("-"):
            if which == "24":
                runs[order, which] = _run_case(d2, c24, b24)
            else:
                runs[order, which] = _run_arrays(d2, c16, b16["recs"], b16["fs"], b16["params"])
        d2.close()
    _assert_same_runs(runs["24-16", "24"], runs["16-24", "24"], "i24 after int16", keys=ALL)
    _assert_same_runs(runs["24-16", "16"], runs["16-24", "16"], "int16 after i24", keys=ALL)
    _check_against_oracle(c24, b24, runs["16-24", "24"])
    _check_against_oracle(c16, b16, runs["24-16", "16"])


@pytest.mark.gpu
def test_host_layers(det, tmp_path):
    """Detector.run_host on Pcm24 equals Detector.run on the same bytes; a
    batch is one format; analyze_wav_files with packed24=True gives the
    results of packed24=False on written 24-bit WAVs."""
    from scipy.io import wavfile

    from bpm_analysis_amd import dropin
    from bpm_analysis_amd.pcm24 import Pcm24
    c = P24["i24x1/146"]
    b = _batch(c)
    keep = [1, 0, 5]
    recs = [Pcm24(b["bytes"][k]) for k in keep]
    assert all(np.array_equal(r.to_int32(), b["recs"][k]) for r, k in zip(recs, keep))
    got = det.run_host(recs, b["fs"], b["params"], mode="native", want_y=True)
    want = _run24(det, c, [b["bytes"][k] for k in keep], [len(r) for r in recs], b["fs"], b["params"])
    _assert_same_runs(got, want, "run_host", keys=ALL)
    with pytest.raises(ValueError, match="one sample format"):
        det.run_host([recs[0], b["recs"][0]], b["fs"], b["params"], mode="native")
    packed = det.run_host_packed(recs, b["fs"], b["params"], mode="native")
    assert len(packed) == len(recs)
    # files: mono and stereo 24-bit, and an int16 one in the same call
    cs = P24["i24x2/146"]
    bs = _batch(cs)
    paths = []
    for i, (fs, x) in enumerate([(b["fs"], b["recs"][1]), (b["fs"], b["recs"][5]), (bs["fs"], bs["recs"][1])]):
        paths.append(str(tmp_path / f"r{i}.wav"))
        raw = _wav24(fs, x)
        with open(paths[-1], "wb") as fh:
            fh.write(raw)
        assert np.array_equal(wavfile.read(paths[-1])[1], x)
    paths.append(str(tmp_path / "r16.wav"))
    wavfile.write(paths[-1], b["fs"], (b["recs"][1] >> 16).astype(np.int16))
    p = dict(b["params"], bpmx_mode="reference")
    plain = dropin.analyze_wav_files(paths, p, str(tmp_path))
    packed24 = dropin.analyze_wav_files(paths, p, str(tmp_path), packed24=True)
    for x, y in zip(plain, packed24):
        assert "error" not in x and "error" not in y
        for key in ("env", "floor", "troughs", "peaks"):
            assert _same(x[key], y[key]), key
        assert (x["sr"], x["flags"]) == (y["sr"], y["flags"])


def _wav24(fs, x):
    import struct
    ch = 1 if x.ndim == 1 else x.shape[1]
    data = _pack(x).tobytes()
    fmt = struct.pack("<HHIIHH", 1, ch, fs, fs * ch * 3, ch * 3, 24)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data + \
        (b"\x00" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body
