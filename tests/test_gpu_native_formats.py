"""Native mode's envelope over every sample format, block-kernel route and
edge: the cases of tests/test_native_plan.py's NATIVE_CASES, which that module
keeps a cover of the plan's branches without a GPU.

A case is one ragged batch in one device buffer, with 64 guard elements of the
format's largest finite value before and after it: a recording of 15 blocks
(a partial tile only, one tail sample), recordings of m bt, m bt + 1 and
(m + 1) bt - 1 blocks with tails of ds, 1 and 2 samples, a long one (about
4.7 s at the decimated rate of 320 Hz) with a tail near ds / 2, and one of
15 ds frames, which is too short (see case_lengths).  Samples and edges are
tests/native_cases.py's.

Conditions on the inputs, asserted on the CPU before any comparison, with
y_cast the oracle's y for the same samples cast to float64 first and
D = max |y_oracle - y_cast| / max |y_oracle|:
* mono u8 / int16 / int32: D >= 1e-3 for every recording: the odd
  extension's wrap-around decides the result, so a head or a tail extended
  without it is far outside the bound;
* float32: D >= 3e-9 over the case, and then the GPU must be within a tenth
  of max |y_oracle - y_cast| (over the case, and per recording wherever
  that recording's own D reaches 3e-9): a kernel that extends or averages in
  double misses that by a factor of ten, with no absolute number involved;
* multi-channel integers: y_oracle equals y_cast (the float64 mean does not
  wrap), while channel 0 alone has D >= 1e-3: a kernel that wraps there fails
  the bound.

Per active recording: sr and lengths; max |y - y_oracle| <= 1e-9 max
|y_oracle| and the same for env (the project's native bound, as in
test_native_mode_golden); floor, troughs, peaks, raw-trough count and flags
equal the oracle's env-level functions on the GPU's own envelope bit for bit;
a second run without y is bit-identical.  int16 cases also run with
BPMX_OPT_NATIVE_F64 and agree within 1e-12 of scale (the bound of
test_native_dma_block_kernel).  The largest errors per (route, format) are
recorded (record_property); DESIGN.md lists what an MI355X gave."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import native_cases as NC
from tests.test_gpu_hilbert_lengths import _oracle_answer
from tests.test_gpu_params import F_TOO_SHORT, _check, _same
from tests.test_native_plan import CASES, NATIVE_CASES, OPT_NATIVE_F64, SAME_TABLE_PAIRS, case_lengths

TOL = 1e-9                        # native mode's bound on y and env against the scipy composition
TOL_F64 = 1e-12                   # between block kernels (their tile lengths differ, so the scans round differently)
D_INT, D_F32, F32_SHARE = 1e-3, 3e-9, 0.1
GUARD = 64
SEED0 = 7000


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


_batches = {}


def _batch(c):
    """A case's recordings and the oracle's answers, made once per module."""
    if c.name not in _batches:
        fs, p = NC.rate(c.ds), NC.params(c.ds)
        d = O.derive(fs, p)
        assert (d.ds, d.sr, d.env_w) == (c.ds, 320, 32)
        recs = [NC.recording(c.dtype, c.ch, n, fs, SEED0 + i) for i, n in enumerate(case_lengths(c))]
        ref = []
        for x in recs[:-1]:
            env, y = O.preprocess_native(x, d, return_y=True)
            ref.append(dict(env=env, y=y, y_cast=NC.cast_y(x, d),
                            y0_d=None if c.ch == 1 else NC.discrimination(
                                O.preprocess_native(np.ascontiguousarray(x[:, 0]), d, return_y=True)[1],
                                NC.cast_y(x[:, 0], d))))
        assert -(-recs[-1].shape[0] // c.ds) == 15             # the inactive one: nd <= 15, the library's F_TOO_SHORT
        _batches[c.name] = dict(fs=fs, params=p, d=d, recs=recs, ref=ref)
    return _batches[c.name]


def _run(det, c, recs, fs, params, want_y=True, opt=None):
    """The batch behind GUARD + c.off guard elements and before GUARD more."""
    import torch
    dt = recs[0].dtype
    top = np.iinfo(dt).max if dt.kind in "iu" else np.finfo(dt).max
    flat = np.concatenate([np.full(GUARD + c.off, top, dt)] + [r.reshape(-1) for r in recs] + [np.full(GUARD, top, dt)])
    lens = [r.shape[0] for r in recs]
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = torch.from_numpy(flat).to(det.device)
    assert dev.data_ptr() % 16 == 0
    pcm = dev[GUARD + c.off:GUARD + c.off + int(fo[-1]) * c.ch]
    res = det.run(pcm, fo, fs, params, mode="native", channels=c.ch, want_y=want_y,
                  options=c.opt if opt is None else opt)
    torch.cuda.synchronize()
    out = res.to_host()
    del dev
    return out


def _assert_inputs_discriminate(c, ref):
    """The module docstring's conditions on the inputs."""
    integer, mono = c.dtype in ("u8", "i16", "i32"), c.ch == 1
    for k, r in enumerate(ref):
        dist = NC.discrimination(r["y"], r["y_cast"])
        if integer and mono:
            assert dist >= D_INT, (c.name, k, dist)
        elif integer:
            assert np.array_equal(r["y"], r["y_cast"]) and r["y0_d"] >= D_INT, (c.name, k, r["y0_d"])
        elif c.dtype == "f64":
            assert np.array_equal(r["y"], r["y_cast"]), (c.name, k)
    if c.dtype == "f32":
        diff = max(float(np.max(np.abs(r["y"] - r["y_cast"]))) for r in ref)
        dist = diff / max(float(np.max(np.abs(r["y"]))) for r in ref)
        print(f"{c.name}: D = {dist:.3e}")
        assert dist >= D_F32, (c.name, dist)
        return diff
    return None


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _check_against_oracle(c, b, res, worst=None):
    """sr, lengths, the two bounds and (float32) the share of the distance to
    y_cast, per active recording; the inactive one has no outputs."""
    ref, diff32 = b["ref"], None
    if c.dtype == "f32":
        diff32 = max(float(np.max(np.abs(r["y"] - r["y_cast"]))) for r in ref)
    assert len(res) == len(ref) + 1
    for k, (r, o) in enumerate(zip(res, ref)):
        assert r["sr"] == b["d"].sr == 320 and r["flags"] & F_TOO_SHORT == 0
        assert r["y"].size == r["env"].size == o["y"].size == -(-b["recs"][k].shape[0] // c.ds), (c.name, k)
        ey, ee = _rel(r["y"], o["y"]), _rel(r["env"], o["env"])
        print(f"{c.name} [{c.route}] recording {k} (nd {o['y'].size}): y {ey:.3e} env {ee:.3e}")
        if worst is not None:
            worst["y"], worst["env"] = max(worst["y"], ey), max(worst["env"], ee)
        assert ey <= TOL and ee <= TOL, (c.name, k, ey, ee)
        if diff32 is not None:
            err = float(np.max(np.abs(r["y"] - o["y"])))
            own = float(np.max(np.abs(o["y"] - o["y_cast"])))
            assert err <= F32_SHARE * diff32, (c.name, k, err, diff32)
            if own >= D_F32 * float(np.max(np.abs(o["y"]))):
                assert err <= F32_SHARE * own, (c.name, k, err, own)
    _assert_inactive(res[-1], c.name)


def _assert_inactive(r, what):
    assert r["flags"] & F_TOO_SHORT, what
    assert r["env"].size == 0 and (r["y"] is None or r["y"].size == 0), what
    assert len(r["troughs"]) == 0 and len(r["peaks"]) == 0 and r["n_raw_troughs"] == 0, what
    assert r["floor"].size == 0, what


def _assert_same_runs(a, b, what, keys=("env", "floor", "troughs", "peaks")):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for key in keys:
            assert _same(x[key], y[key]), (what, k, key)
        assert x["flags"] == y["flags"] and x["n_raw_troughs"] == y["n_raw_troughs"], (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in NATIVE_CASES])
def test_native_case(det, record_property, name):
    c = CASES[name]
    b = _batch(c)
    _assert_inputs_discriminate(c, b["ref"])
    worst = {"y": 0.0, "env": 0.0}
    with_y = _run(det, c, b["recs"], b["fs"], b["params"])
    _check_against_oracle(c, b, with_y, worst)
    record_property(f"max_rel_err_y[{c.route} {c.dtype}]", worst["y"])
    record_property(f"max_rel_err_env[{c.route} {c.dtype}]", worst["env"])
    # without y (k_hilbert_env makes yd of the fused recordings' full tiles itself when bt is even)
    plain = _run(det, c, b["recs"], b["fs"], b["params"], want_y=False)
    _assert_same_runs(plain, with_y, name)
    # detection on the GPU's own envelope
    for k, r in enumerate(plain[:-1]):
        _check(r, _oracle_answer(np.ascontiguousarray(r["env"]), b["params"], b["fs"]), (name, k))
    if c.dtype == "i16":
        f64 = _run(det, c, b["recs"], b["fs"], b["params"], opt=c.opt | OPT_NATIVE_F64)
        for k, (x, y) in enumerate(zip(with_y[:-1], f64[:-1])):
            sy, se = np.max(np.abs(y["y"])), np.max(np.abs(y["env"]))
            assert np.max(np.abs(x["y"] - y["y"])) <= TOL_F64 * sy, (name, k)
            assert np.max(np.abs(x["env"] - y["env"])) <= TOL_F64 * se, (name, k)
        _assert_inactive(f64[-1], name)


@pytest.mark.gpu
def test_inactive_recordings_only(det):
    """A batch without an active recording: no tile, no block launch, every
    recording F_TOO_SHORT with counts 0 and empty slices."""
    c = CASES["i32x2"]
    fs, p = NC.rate(c.ds), NC.params(c.ds)
    recs = [NC.recording(c.dtype, c.ch, n, fs, SEED0 + 50 + i) for i, n in enumerate((15 * c.ds, 14 * c.ds + 1, 40, c.ds))]
    det.profile_only("")
    det.profile(True)
    res = _run(det, c, recs, fs, p)
    det.profile(False)
    prof = det.profile_read()
    assert "k_native_blocks" not in prof and "k_native_yd" not in prof, prof
    assert len(res) == 4
    for k, r in enumerate(res):
        _assert_inactive(r, k)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SAME_TABLE_PAIRS, ids=["+".join(p) for p in SAME_TABLE_PAIRS])
def test_same_tables_either_order(pair):
    """Two cases that share ds and bt (the table cache's key but for key16)
    and differ in route or format, back to back in both orders on a fresh
    context each: the same bits, and within the bound."""
    from bpm_analysis_amd.engine import Detector
    a, b = (CASES[n] for n in pair)
    runs = {}
    for order in ((a, b), (b, a)):
        d2 = Detector(0)
        for c in order:
            bb = _batch(c)
            runs[order[0].name, c.name] = _run(d2, c, bb["recs"], bb["fs"], bb["params"])
        d2.close()
    for c in (a, b):
        first, second = runs[c.name, c.name], runs[(b if c is a else a).name, c.name]
        _assert_same_runs(first, second, (pair, c.name), keys=("y", "env", "floor", "troughs", "peaks"))
        _check_against_oracle(c, _batch(c), second)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32x2", "i32x1"])
def test_recordings_do_not_leak_into_each_other(det, name):
    """The second recording's first 17 frames at the format's largest value
    and its last 17 at the smallest (+-1e30 for float32; no NaN or Inf
    anywhere): every other recording's outputs are bit-identical to the batch
    where that recording is zeros."""
    c = CASES[name]
    b = _batch(c)
    hot, cold = [r.copy() for r in b["recs"]], [r.copy() for r in b["recs"]]
    dt = hot[1].dtype
    lo, hi = (-1e30, 1e30) if dt.kind == "f" else (np.iinfo(dt).min, np.iinfo(dt).max)
    hot[1][:NC.EDGE], hot[1][-NC.EDGE:] = hi, lo
    cold[1][...] = 0
    rh = _run(det, c, hot, b["fs"], b["params"])
    rc = _run(det, c, cold, b["fs"], b["params"])
    assert np.all(np.isfinite(rh[1]["y"])) and np.all(np.isfinite(rh[1]["env"]))
    assert not _same(rh[1]["y"], rc[1]["y"])
    keep = [k for k in range(len(hot)) if k != 1]
    _assert_same_runs([rh[k] for k in keep], [rc[k] for k in keep], name, keys=("y", "env", "floor", "troughs", "peaks"))
    _check_against_oracle(c, dict(b, recs=[b["recs"][k] for k in keep], ref=[b["ref"][k] for k in keep if k < len(b["ref"])]),
                          [rh[k] for k in keep])
