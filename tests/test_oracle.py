"""The CPU oracle against the reference's golden vectors (pins the oracle)."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import goldens as G


@pytest.mark.parametrize("name", G.names(kind="pcm"))
def test_oracle_pcm_goldens(name):
    g = G.load(name)
    mode = str(g["mode"])
    o = O.detect(g["pcm"], int(g["fs"]), g["params"], mode=mode)
    assert o["sr"] == int(g["sr"])
    if mode == "reference":
        # bit-exact: preprocess_audio, filtfilt, noise floor
        assert np.array_equal(o["y"], g["y"])
        assert np.array_equal(o["env"], g["env"])
        assert np.array_equal(o["floor"], g["floor"], equal_nan=True)
    else:
        # native mode oracle: sosfiltfilt bit-exact, hilbert via numpy.fft (<= 1e-12 rel)
        assert np.array_equal(o["y"], g["y"])
        scale = np.max(np.abs(g["env"]))
        assert np.max(np.abs(o["env"] - g["env"])) <= 1e-12 * scale
        assert np.allclose(o["floor"], g["floor"], rtol=1e-10, atol=0)
    assert np.array_equal(o["troughs"], g["troughs"])
    assert np.array_equal(o["peaks"], g["peaks"])
    assert o["flags"] == int(g["flags"])


@pytest.mark.parametrize("name", [n for n in G.names(kind="env") if not n.startswith("env_ties")])
def test_oracle_env_goldens(name):
    g = G.load(name)
    d = G.env_derived(g)
    floor, tr, flags = O.noise_floor(g["env"], d, g["params"])
    assert np.array_equal(floor, g["floor"], equal_nan=True)
    assert np.array_equal(tr, g["troughs"])
    assert flags == int(g["flags"])
    pk, tie = O.raw_peaks(g["env"], floor, d, g["params"], return_tie=True)
    assert np.array_equal(pk, g["peaks"])
    assert not tie


@pytest.mark.parametrize("name", G.names(kind="env", prefix="env_ties"))
def test_oracle_tie_goldens(name):
    """Envelopes with equal-height extrema closer than find_peaks' distance.
    (1) The restatement with numpy's own argsort order in the distance filter
    reproduces the reference's raw troughs and raw peaks exactly, which pins
    every other step of the oracle's find_peaks on these inputs.  (2) The
    stable order (the oracle's and the kernels' convention) differs from it
    here, and the decisive-tie report is set: on every tie golden, for the
    troughs and for the peaks wherever their answers differ."""
    g = G.load(name)
    d = G.env_derived(g)
    env, p = g["env"], g["params"]
    qt = O.quantile(env, p["trough_prominence_quantile"])
    qp = O.quantile(env, p["peak_prominence_quantile"])
    assert np.array_equal(O.find_peaks_numpy_order(env, distance=d.distance, prominence=qt, negate=True),
                          g["raw_troughs"])
    assert np.array_equal(O.find_peaks_numpy_order(env, height=g["floor"], distance=d.distance, prominence=qp),
                          g["peaks"])
    raw, ttie = O.find_peaks(env, distance=d.distance, prominence=qt, negate=True, return_tie=True)
    assert ttie and not np.array_equal(raw, g["raw_troughs"])
    _, _, flags = O.noise_floor(env, d, p)
    assert flags & O.F_TROUGH_TIE
    pk, ptie = O.raw_peaks(env, g["floor"], d, p, return_tie=True)
    assert ptie or np.array_equal(pk, g["peaks"])
    # (3) the whole noise floor in numpy's order (the GPU tie resolution's
    # checker): the reference's troughs and floor, bit for bit
    nf, nt, nfl, nraw = O.noise_floor_numpy_order(env, d, p)
    assert np.array_equal(nraw, g["raw_troughs"])
    assert np.array_equal(nt, g["troughs"])
    assert np.array_equal(nf, g["floor"], equal_nan=True)
    assert (nfl & 3) == (int(g["flags"]) & 3)


def test_noise_floor_from_raw_matches_c_restatement():
    """noise_floor_from_raw (the Python composition behind the numpy-order
    floor) equals bpmx_oracle.c's noise floor when both start from the same raw
    troughs (the stable order's, on every golden envelope without a tie)."""
    for name in [n for n in G.names(kind="env") if not n.startswith("env_ties")]:
        g = G.load(name)
        d = G.env_derived(g)
        env, p = g["env"], g["params"]
        raw = O.find_peaks(env, distance=d.distance, negate=True,
                           prominence=O.quantile(env, p["trough_prominence_quantile"]))
        f1, t1, fl1 = O.noise_floor(env, d, p)
        f2, t2, fl2 = O.noise_floor_from_raw(env, raw, d, p)
        assert np.array_equal(f1, f2, equal_nan=True), name
        assert np.array_equal(t1, t2), name
        assert (fl1 & 7) == fl2, name


def test_tie_report_is_exact():
    """The report is set iff some argsort order of the equal heights changes the
    distance filter's outcome: checked against every tie order (permutations
    of each equal-height block) on small random quantized envelopes."""
    import itertools
    import math
    rng = np.random.default_rng(7)
    for trial in range(300):
        n = int(rng.integers(20, 60))
        x = rng.integers(0, 4, n).astype(np.float64)
        cand = O.find_peaks(x)
        if cand.size < 2:
            continue
        dist = int(rng.integers(2, 8))
        _, tie = O.find_peaks(x, distance=dist, return_tie=True)
        pr = x[cand]
        outcomes = set()
        levels = sorted(set(pr.tolist()))
        blocks = [np.flatnonzero(pr == v) for v in levels]
        if np.prod([float(math.factorial(len(b))) for b in blocks]) > 5000:
            continue
        for perms in itertools.product(*[itertools.permutations(b) for b in blocks]):
            order = np.concatenate([np.array(pp, dtype=np.int64) for pp in perms])   # ascending priority
            keep = np.ones(cand.size, dtype=bool)
            for i in range(cand.size - 1, -1, -1):
                j = order[i]
                if not keep[j]:
                    continue
                for k in range(cand.size):
                    if k != j and abs(int(cand[k]) - int(cand[j])) < dist:
                        keep[k] = False
            outcomes.add(tuple(cand[keep].tolist()))
        assert tie == (len(outcomes) > 1), (x.tolist(), dist)


def _grid_envelopes():
    """Three seeded 6000-sample envelopes without equal values (checked by the
    test): rough, beats on noise, a slow wander."""
    rng = np.random.default_rng(302)
    n = 6000
    t = np.arange(n)
    beat = np.maximum(0.0, np.sin(2 * np.pi * t / 250.0)) ** 8
    return [rng.random(n) ** 3 * 1000 + 50 * beat,
            300 * beat + rng.random(n) + 20,
            200 + 80 * np.sin(t / 700.0) + 300 * beat + rng.random(n)]


GRID_DISTANCES = [1, 2, 3, 15, 40, 128, 129, 300, 906, 7000]
GRID_LEVELS = [0.0, 0.05, 0.2, 0.5, 0.9, 0.999, 1.0]


def _grid_windows(n):
    return [3, 4, 5, 6, 63, 64, 65, 151, 302, 3019, 3020, n - 1, n, n + 1, 2 * n + 1, 20000]


def test_oracle_matches_libraries_off_the_defaults():
    """The oracle's find_peaks, interp_dense + rolling_quantile and quantile
    against the library calls the reference makes (scipy.signal.find_peaks,
    pandas' reindex + interpolate, which leaves NaN before the first trough,
    its centred rolling quantile with bfill / ffill, np.quantile), bit for
    bit, over distances, windows and levels far from the defaults: distance 1
    (no filter) to beyond the envelope, windows of 3-5 samples (NaN edges),
    even and odd, up to more than twice the envelope, levels 0, 1 and close
    to 1."""
    import pandas as pd
    from scipy.signal import find_peaks
    for env in _grid_envelopes():
        n = env.size
        assert np.unique(env).size == n                     # no equal heights: the tie order decides nothing
        prom = float(np.quantile(env, 0.1))
        for q in GRID_LEVELS:
            assert O.quantile(env, q) == np.quantile(env, q)
        for dist in GRID_DISTANCES:
            for neg in (False, True):
                x = -env if neg else env
                for kw in (dict(distance=dist), dict(distance=dist, prominence=prom)):
                    got, tie = O.find_peaks(env, negate=neg, return_tie=True, **kw)
                    assert np.array_equal(got, find_peaks(x, **kw)[0]), (dist, neg, kw)
                    assert not tie
            floor = np.full(n, np.quantile(env, 0.3))
            assert np.array_equal(O.find_peaks(env, height=floor, distance=dist, prominence=prom),
                                  find_peaks(env, height=floor, distance=dist, prominence=prom)[0])
        for dist in (2, 15, 300):
            tr = find_peaks(-env, distance=dist, prominence=prom)[0]
            dense = O.interp_dense(tr, env)
            s = pd.Series(index=tr, data=env[tr]).reindex(np.arange(n)).interpolate()
            assert np.isnan(s.values[:tr[0]]).all() and not np.isnan(s.values[tr[0]:]).any()
            assert np.array_equal(dense, s.values, equal_nan=True)
            for w in _grid_windows(n):
                roll = s.rolling(window=w, min_periods=3, center=True)
                for q in GRID_LEVELS:
                    want = roll.quantile(q).bfill().ffill().values
                    assert np.array_equal(O.rolling_quantile(dense, w, 3, q), want, equal_nan=True), (dist, w, q)


@pytest.mark.parametrize("name", G.names(kind="env", prefix="env_params"))
def test_param_fixtures_exact_settings_and_tie_free(name):
    """The env_params_* fixtures: the `*_sec` settings give the intended
    integers through both derivations (the oracle's and the package's), at
    least one setting is off its default, and no height tie decides anything
    (numpy's argsort order and the stable order give the same troughs, floor
    and peaks), so the reference's recorded outputs pin one answer."""
    from bpm_analysis_amd import design
    from tests.golden import inputs as I
    g = G.load(name)
    env, p, sr = g["env"], g["params"], int(g["sr"])
    d = G.env_derived(g)
    dd = design.detect_design(sr, p)
    assert (dd.distance, dd.noise_window) == (d.distance, d.noise_window)
    over = I.env_cases()[name][2]
    want = {"min_peak_distance_sec": d.distance, "noise_window_sec": d.noise_window}
    for key, got in want.items():
        if key in over:
            assert over[key] == I.sec_for(got, sr)
    assert over and all(p[k] != G.BASE_PARAMS[k] for k in over)
    raw, ttie = O.find_peaks(env, distance=d.distance, negate=True, return_tie=True,
                             prominence=O.quantile(env, p["trough_prominence_quantile"]))
    floor, tr, flags = O.noise_floor(env, d, p)
    pk, ptie = O.raw_peaks(env, floor, d, p, return_tie=True)
    assert not ttie and not ptie
    nf, nt, nfl, nraw = O.noise_floor_numpy_order(env, d, p)
    assert np.array_equal(nraw, raw) and np.array_equal(nt, tr) and np.array_equal(nf, floor, equal_nan=True)
    npk = O.find_peaks_numpy_order(env, height=floor, distance=d.distance,
                                   prominence=O.quantile(env, p["peak_prominence_quantile"]))
    assert np.array_equal(npk, pk)


def test_param_fixtures_reach_their_branches():
    """What each env_params_* fixture is for, read off the reference's outputs."""
    g = {n: G.load(n) for n in G.names(kind="env", prefix="env_params")}
    d = {n: G.env_derived(v) for n, v in g.items()}
    assert len(g) == 7
    assert d["env_params_distance1"].distance == 1
    assert np.min(np.diff(g["env_params_distance1"]["peaks"])) < 15      # closer than the default distance keeps
    assert d["env_params_distance453"].distance == 453
    assert d["env_params_window3"].noise_window == 3 and not np.isnan(g["env_params_window3"]["floor"]).any()
    w = g["env_params_window151_q50"]
    assert d["env_params_window151_q50"].noise_window == 151 and w["params"]["noise_floor_quantile"] == 0.5
    assert g["env_params_q0"]["params"]["noise_floor_quantile"] == 0.0
    assert g["env_params_q1_levels"]["params"]["noise_floor_quantile"] == 1.0
    s = g["env_params_static_q10"]
    assert int(s["flags"]) == 1 and len(s["troughs"]) < 5
    assert np.all(s["floor"] == np.quantile(s["env"], 0.1))


def test_oracle_vulpine_known_answer():
    """Labeler-recipe envelope of the committed filtered WAV reproduces every raw
    peak index of samples/vulpine_Debug_Log.md (heartbeat_labeler.py:63-67)."""
    g = G.load("vulpine")
    w = g["pcm"]
    env = O.rolling_mean(np.abs(w).astype(np.float64), int(g["fs"]) // 10, 1)
    d = O.derive(302 * 146, dict(g["params"]))
    d.sr, d.distance, d.noise_window = 302, 15, 3020
    floor, tr, _ = O.noise_floor(env, d, g["params"])
    pk = O.raw_peaks(env, floor, d, g["params"])
    assert np.array_equal(pk, g["log_peaks"])
    assert len(np.intersect1d(tr, g["log_troughs"])) >= 1345  # 4 off by int16 quantisation
    # and the reference pipeline run on the same WAV
    o = O.detect(w, int(g["fs"]), g["params"])
    assert np.array_equal(o["env"], g["env"])
    assert np.array_equal(o["troughs"], g["troughs"])
    assert np.array_equal(o["peaks"], g["peaks"])


def test_short_input_raises():
    pcm = O.synth(1, 146 * 15, 44100, 1)
    with pytest.raises(ValueError):
        O.detect(pcm, 44100, G.BASE_PARAMS)


def test_oracle_under_sanitizers(tmp_path):
    """SURVEY.md section 5 (race detection / sanitizers): the C restatement under
    ASan + UBSan on synthetic recordings (reference and native ordering,
    stereo, padlen rejects) and envelope edge cases (constant, ramps, windows
    longer than the recording).  Any invalid access, leak or UB fails."""
    import shutil
    import subprocess
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("gcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "sanitize_driver")
    cmd = [cc, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-ffp-contract=off", "-std=c11", "-o", exe, os.path.join(here, "sanitize_driver.c"), "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in (b.stderr or ""):
        pytest.skip("sanitizer runtime not available: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SANITIZE OK" in r.stdout


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["u8", "i16", "i32", "f32", "f64"])
def test_native_y_is_scipys_in_every_sample_format(dtype, ch):
    """preprocess_native's decimated signal is scipy.signal.sosfiltfilt of the
    same-dtype array (np.mean over the channels first, as the reference
    forms it), decimated, bit for bit: the int16 goldens pin the oracle for
    int16 only, and odd_ext's arithmetic in the array's dtype (wrap-around for
    mono integers, float32 rounding, neither for a float64 mean) differs per
    format.  Recordings with tests/native_cases.py's edges, on which that
    arithmetic decides the result: asserted through the same samples cast to
    float64 first."""
    from scipy.signal import sosfiltfilt
    from tests import native_cases as NC
    ds = 146
    fs = NC.rate(ds)
    d = O.derive(fs, NC.params(ds))
    assert (d.ds, d.sr, d.env_w) == (ds, 320, 32)
    for i, n in enumerate((15 * ds + 1, 16 * ds, 41 * ds + 73)):
        x = NC.recording(dtype, ch, n, fs, 4100 + i)
        assert x.dtype == NC.NP_DT[dtype] and x.shape == ((n,) if ch == 1 else (n, ch))
        env, y = O.preprocess_native(x, d, return_y=True)
        work = x if ch == 1 else np.mean(x, axis=1)
        assert work.dtype == (x.dtype if ch == 1 or dtype == "f32" else np.float64)
        want = sosfiltfilt(d.sos, work)[::ds]
        assert y.dtype == want.dtype == np.float64 and np.array_equal(y, want), (n, dtype, ch)
        dist = NC.discrimination(y, NC.cast_y(x, d))
        if dtype == "f64" or (ch > 1 and dtype != "f32"):
            assert dist == 0.0                                  # no wrap, no rounding: the cast changes nothing
        elif dtype == "f32":
            assert dist > 0.0
        else:
            assert dist >= 1e-3, dist
