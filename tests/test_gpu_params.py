"""GPU parity of the detection stages away from the default settings.

find_peaks' distance, the noise window and the three quantile levels select
most of the branches in the detection kernels and in the host's kernel
selection.  Every test here runs ragged batches of envelopes through
``run_env_host`` (or short PCM recordings through native mode) over grids of
those settings and compares floor, troughs, raw peaks, the raw-trough count and
the flags with the oracle, bit for bit.

The grids are kept honest on the CPU, by assertions made before anything is
compared (``_assert_sensitive``, ``_neighbour_shares``): each setting is hit
exactly (``sec_for``), the oracle's answer changes when a grid value moves by
one, and the paths the grids are meant to reach are reached."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import goldens as G
from tests.golden.inputs import _vshape, sec_for

SR = 302
FALLBACK_BITS = 3
TIE_BITS = O.F_TROUGH_TIE | O.F_PEAK_TIE
FLAG_MASK = FALLBACK_BITS | 4 | TIE_BITS     # static / draft / all-NaN fallbacks and the decisive-tie reports
F_TOO_SHORT, F_BAD_WINDOW = 8, 16

# kernel constants the grids straddle (bpmx_kernels.h)
FL_MC, FPL_NMIN, WM_MMAX, WM_TRMAX, RQ_T = 3072, 65536, 18432, 512, 256
DB_TRMAX, DB_LOCAL_M = 2040, 512


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _beat(n, period=250.0):
    return np.maximum(0.0, np.sin(2 * np.pi * np.arange(n) / period)) ** 8


def _params(distance=15, window=3020, **over):
    """BASE_PARAMS with `distance` and `noise_window` hit exactly, checked
    through both derivations (the oracle's and the package's)."""
    from bpm_analysis_amd import design
    p = dict(G.BASE_PARAMS, min_peak_distance_sec=sec_for(distance, SR), noise_window_sec=sec_for(window, SR))
    p.update(over)
    d, dd = G.env_derived({"params": p, "sr": SR}), design.detect_design(SR, p)
    assert d.distance == dd.distance == distance and d.noise_window == dd.noise_window == window
    return p


_answers = {}


@pytest.fixture(autouse=True)
def _drop_answers():
    yield
    _answers.clear()


def _answer(env, params, sr_fs=None):
    """The oracle's env-level answer, memoised per envelope object and settings
    for the length of one test (an entry keeps its envelope alive, so an id
    is not reused while it is a key).
    sr_fs: derive from this PCM rate instead of the 302 Hz envelope rate."""
    key = (id(env), sr_fs, tuple(sorted(params.items())))
    if key not in _answers:
        d = G.env_derived({"params": params, "sr": SR}) if sr_fs is None else O.derive(sr_fs, params)
        floor, tr, fl = O.noise_floor(env, d, params)
        pk, ptie = O.raw_peaks(env, floor, d, params, return_tie=True)
        raw = O.find_peaks(env, distance=d.distance, negate=True,
                           prominence=O.quantile(env, params["trough_prominence_quantile"]))
        _answers[key] = dict(env=env, floor=floor, troughs=tr, peaks=pk, n_raw=len(raw),
                             flags=fl | (O.F_PEAK_TIE if ptie else 0))
    return _answers[key]


def _check(r, o, what, peaks=True):
    assert _same(r["floor"], o["floor"]), ("floor", what)
    assert _same(r["troughs"], o["troughs"]), ("troughs", what)
    assert r["n_raw_troughs"] == o["n_raw"], ("n_raw_troughs", what)
    mask = FLAG_MASK if peaks else FLAG_MASK & ~O.F_PEAK_TIE
    assert (r["flags"] & mask) == (o["flags"] & mask), ("flags", what, r["flags"], o["flags"])
    assert r["flags"] & (F_TOO_SHORT | F_BAD_WINDOW) == 0, ("flags", what)
    if peaks:
        assert _same(r["peaks"], o["peaks"]), ("peaks", what)


def _check_equal_runs(a, b, what):
    for x, y in zip(a, b):
        for k in ("floor", "troughs", "peaks"):
            assert _same(x[k], y[k]), (k, what)
        assert x["flags"] == y["flags"] and x["n_raw_troughs"] == y["n_raw_troughs"], what


def _differs(a, b):
    return not (_same(a["floor"], b["floor"]) and _same(a["troughs"], b["troughs"]) and
                _same(a["peaks"], b["peaks"]) and a["n_raw"] == b["n_raw"])


def _assert_sensitive(envs, values, make, lowest, same):
    """An off-by-one in a kernel bound cannot pass: for every grid value v the
    oracle's answer at v differs from its answers at v - 1 and at v + 1 on at
    least one envelope of the batch.  Two exceptions, both by proof, not by
    observation: a neighbour below `lowest` is no valid setting (find_peaks and
    pandas raise), and where `same(v, w)` says that the answer cannot depend
    on the value (the caller gives the argument) it is asserted to be equal."""
    for v in values:
        for w in (v - 1, v + 1):
            if w < lowest:
                continue
            if same(min(v, w), max(v, w)):
                assert not any(_differs(_answer(e, make(v)), _answer(e, make(w))) for e in envs[:2]), (v, w)
                continue
            assert any(_differs(_answer(e, make(v)), _answer(e, make(w))) for e in envs), (v, w)


def _same_distance(nmax):
    """Local maxima are at least 2 samples apart, so distances 1 and 2 remove
    nothing; they all lie in [1, n - 2], so from n - 2 on every pair of them is
    closer than the distance and only the highest stays."""
    return lambda lo, hi: hi <= 2 or lo >= nmax - 2


def _same_window(nmax):
    """From 2 n - 1 on, every centred window holds the whole recording."""
    return lambda lo, hi: lo >= 2 * nmax - 1


def _spike_pairs(distances, seed):
    """An envelope on which find_peaks' answer changes at every distance d and
    d + 1 of the grid: for each spacing s in {d - 1, d} a pair of one-sample
    spikes exactly s apart on low noise, the first the taller.  Pairs stand in
    ascending order of spacing and of height, each followed by a gap of s + 2,
    so within s + 1 of a pair only lower spikes stand: the taller spike always
    stays, the other one stays at distance <= s and goes at s + 1."""
    spacings = sorted({s for d in distances for s in (d - 1, d) if s >= 2})
    pos, val, x = [], [], 20
    for i, s in enumerate(spacings):
        pos += [x, x + s]
        val += [1010.0 + 20 * i, 1000.0 + 20 * i]
        x += 2 * s + 2
    env = np.random.default_rng(seed).random(x + 20)
    env[pos] = val
    return env


def _neighbour_shares(env, distance, sign=-1.0):
    """Of find_peaks' candidates (all local maxima of sign * env), the share
    with more than eight higher-priority neighbours within `distance`
    (k_find_peaks_lds lists eight per candidate and scans beyond) and the share
    with such a neighbour more than a signed byte of candidates away (left:
    strictly higher, right: at least as high, as the kernel counts them)."""
    cand = O.find_peaks(env, negate=sign < 0)
    h = sign * env[cand]
    k = np.arange(cand.size)
    off = k[None, :] - k[:, None]
    near = np.abs(cand[None, :] - cand[:, None]) < distance
    higher = ((off < 0) & (h[None, :] > h[:, None])) | ((off > 0) & (h[None, :] >= h[:, None]))
    nb = near & higher
    return float((nb.sum(1) > 8).mean()), float((nb & ((off < -128) | (off > 127))).any(1).mean())


def _n_extrema(env, sign):
    return len(O.find_peaks(env, negate=sign < 0))


# ----------------------------------------------------------------------------
# find_peaks' distance
# ----------------------------------------------------------------------------
DISTANCES = [1, 2, 3, 9, 15, 40, 128, 129, 400, 906, 9500]


@functools.lru_cache(maxsize=None)
def _distance_envelopes():
    rng = np.random.default_rng(1906)
    t = np.arange(9000)
    envs = {
        "beat": 300 * _beat(5000) + rng.random(5000) + 20,
        "rough": rng.random(6000) ** 3 * 1000 + 50 * _beat(6000),
        "dense": rng.random(9000) * 10,                               # just under FL_MC maxima
        "over": rng.random(8000) * 10 + 6 * (t[:8000] % 2),           # > FL_MC maxima: handed to k_find_peaks
        "wander": 200 + 80 * np.sin(t[:7000] / 700.0) + 300 * _beat(7000) + rng.random(7000),
        "quant": np.round(5 + 100 * np.sin(t[:4000] / 40.0) ** 2 + rng.random(4000) * 6) / 3.0,   # height ties
        "pairs": _spike_pairs([k for k in DISTANCES if k < 9000], 7),
    }
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in envs.items()}


@pytest.mark.gpu
def test_distance_sweep(det):
    """Distances 1 (no filter: ST_KEPT straight from the height filter) to
    beyond the recording, through k_find_peaks_lds (up to eight listed
    neighbours, the full scan beyond eight or beyond a signed byte) and
    k_find_peaks (BPMX_OPT_PEAKS_GLOBAL, and the > FL_MC-maxima envelope), with
    the decisive-tie report on a quantised envelope and its resolution in
    numpy's order at two large distances."""
    from bpm_analysis_amd import _native as N
    from tests.test_gpu_parity import _numpy_order_answer
    E = _distance_envelopes()
    envs = list(E.values())
    nmax = max(e.size for e in envs)
    assert DISTANCES[-1] > nmax
    for sign in (-1.0, 1.0):
        assert 2900 <= _n_extrema(E["dense"], sign) <= FL_MC
        assert _n_extrema(E["over"], sign) > FL_MC
    make = lambda k: _params(distance=k)
    _assert_sensitive(envs, DISTANCES, make, lowest=1, same=_same_distance(nmax))
    many, far = {}, {}
    for k in DISTANCES:
        many[k], far[k] = zip(*[_neighbour_shares(E[name], k) for name in ("rough", "quant")])
    assert all(max(many[k]) == 0.0 and max(far[k]) == 0.0 for k in (1, 2, 3))
    assert max(many[15]) < 0.5 < max(many[40])
    assert max(far[129]) < 0.5 < max(far[906])
    assert max(max(v) for v in many.values()) > 0.5 and max(max(v) for v in far.values()) > 0.5

    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    seen = 0
    for k in DISTANCES:
        p = make(k)
        a = det.run_env_host(envs, SR, p, stages)
        b = det.run_env_host(envs, SR, p, stages, options=N.OPT_PEAKS_GLOBAL)
        _check_equal_runs(a, b, k)
        for name, r in zip(E, a):
            o = _answer(E[name], p)
            _check(r, o, (name, k))
            seen |= o["flags"]
    assert seen & 1 and seen & TIE_BITS                   # the static floor (one trough left) and a tie report ran
    # decisive ties at large distances (most candidates on the full-scan path), re-decided in numpy's order
    for k in (400, 906):
        p = make(k)
        assert _answer(E["quant"], p)["flags"] & TIE_BITS
        assert max(_neighbour_shares(E["quant"], k)) > 0.5
        d = G.env_derived({"params": p, "sr": SR})
        nf, nt, nfl, nraw, npk = _numpy_order_answer(E["quant"], d, p)
        for opt in (0, N.OPT_PEAKS_GLOBAL):
            r = det.run_env_host([E["quant"], E["beat"]], SR, p, stages, options=opt, resolve_ties=True)
            assert _same(r[0]["troughs"], nt) and _same(r[0]["floor"], nf) and _same(r[0]["peaks"], npk)
            assert r[0]["n_raw_troughs"] == len(nraw) and r[0]["flags"] & TIE_BITS == 0
            _check(r[1], _answer(E["beat"], p), ("beat, resolve_ties", k))


# ----------------------------------------------------------------------------
# noise window and noise-floor level, recordings <= WM_MMAX
# ----------------------------------------------------------------------------
N_W = 9000                                   # the length the windows n - 1 ... 2 n + 1 refer to
WINDOWS = [3, 4, 5, 6, 63, 64, 65, 151, 1510, 3019, 3020, N_W - 1, N_W, N_W + 1, 2 * N_W + 1]
LEVELS = [0.0, 0.05, 0.2, 0.5, 0.9, 0.999, 1.0]
WINDOWS_EDGE = [3, 4, 5, 3020, N_W - 1, N_W, N_W + 1, 2 * N_W + 1]       # these also run every kernel variant
LEVELS_EDGE = [0.0, 0.2, 0.999, 1.0]
ROLLQ_VARIANTS = ("OPT_ROLLQ_NOPRUNE", "OPT_DRAFT_FULL", "OPT_ROLLQ_MERGE", "OPT_ROLLQ_GLOBAL")


@functools.lru_cache(maxsize=None)
def _window_envelopes():
    """The families of test_gpu_parity._floor_envelopes, generated here and
    shorter (the oracle's cost is the test's): beats on noise, a ramp, a floor
    with ulp-level differences, random roughness, more than WM_TRMAX troughs,
    a short recording."""
    rng = np.random.default_rng(3020)
    t = np.arange(11000)
    beat = _beat(11000)
    envs = {
        "beat": 300 * beat[:N_W] + rng.random(N_W) + 20,
        "ramp": 10.0 + 0.05 * t[:6000] + 3000 * beat[:6000] + rng.random(6000),
        "ulp": 10.0 + np.spacing(10.0) * rng.integers(0, 5, 5000) + 300 * beat[:5000],
        "rough": rng.random(5000) ** 3 * 1000 + 50 * beat[:5000],
        "many": np.abs(np.sin(t / 6.0)) * 100 + rng.random(11000),
        "short": 300 * beat[:4000] + rng.random(4000) + 20,
    }
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in envs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS)
def test_window_and_level_sweep(det, w):
    """Noise windows of 3 samples (NaN edges, closed by bfill / ffill) to more
    than twice the recording, even and odd, each crossed with noise-floor
    levels 0 to 1, through k_draft_bounds / k_draft_points, k_floor_wm and the
    pruned wavelet matrix; at the boundary values also the unpruned matrix,
    the full draft, the sorted-union kernels (LDS and global) and rejection
    multiplier 1.0, all equal to the default run and to the oracle."""
    import pandas as pd
    from bpm_analysis_amd import _native as N
    E = _window_envelopes()
    envs = list(E.values())
    nmax = max(e.size for e in envs)
    assert E["beat"].size == N_W and nmax <= 18124
    make = lambda w, **kw: _params(window=w, **kw)
    # min_periods = 3 is the smallest window pandas takes
    _assert_sensitive(envs, [w], make, lowest=3, same=_same_window(nmax))
    assert _answer(E["many"], make(3020))["n_raw"] > WM_TRMAX
    if w <= 5:
        # W <= 5 leaves NaN that the fills close: before the first trough's
        # window for each, after the last full window for W = 3
        raw = O.find_peaks(E["beat"], distance=15, negate=True, prominence=O.quantile(E["beat"], 0.1))
        dense = pd.Series(O.interp_dense(raw, E["beat"]))
        nan = np.isnan(dense.rolling(window=w, min_periods=3, center=True).quantile(0.2).values)
        assert nan[raw[0] - 1] and not nan[raw[0] + 2] and nan[-1] == (w == 3)

    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    seen, undecided = 0, 0
    for q in LEVELS:
        p = make(w, noise_floor_quantile=q)
        a = det.run_env_host(envs, SR, p, stages)
        for name, r in zip(E, a):
            _check(r, _answer(E[name], p), (name, w, q))
        if w in WINDOWS_EDGE and q in LEVELS_EDGE:
            for opt in ROLLQ_VARIANTS:
                _check_equal_runs(a, det.run_env_host(envs, SR, p, stages, options=getattr(N, opt)), (w, q, opt))
            p1 = make(w, noise_floor_quantile=q, trough_rejection_multiplier=1.0)
            a1 = det.run_env_host(envs, SR, p1, stages, options=N.OPT_STATS)
            undecided += det.stats()["undecided"]
            for name, r in zip(E, a1):
                o = _answer(E[name], p1)
                _check(r, o, (name, w, q, "multiplier 1.0"))
                seen |= o["flags"]
            _check_equal_runs(a1, det.run_env_host(envs, SR, p1, stages, options=N.OPT_DRAFT_FULL),
                              (w, q, "multiplier 1.0, full draft"))
    if w in WINDOWS_EDGE and w >= 3020:
        assert undecided > 0                              # k_draft_points decided some troughs
    if w == 2 * N_W + 1:
        assert seen & 2                                   # level 0, multiplier 1: only the lowest trough stays


@pytest.mark.gpu
@pytest.mark.parametrize("w", [3, 3020, 7938])
def test_union_kernels_at_level_one(det, w):
    """Regression: noise_floor_quantile = 1.0 through the sorted-union kernels
    (k_rolling_quantile, k_rolling_quantile_g).  The window's k-th sample is
    then its last, and the search for the next one in the window ran off the
    end of the union (an illegal access in the global-scratch kernel, first
    seen at W = 3 with BPMX_OPT_ROLLQ_GLOBAL on the 4000-sample envelope).
    Forced on short recordings, and the default path of one past WM_MMAX."""
    from bpm_analysis_amd import _native as N
    E, L = _window_envelopes(), _long_envelopes()
    p = _params(window=w, noise_floor_quantile=1.0)
    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    for envs, opts in (([E["short"]], (N.OPT_ROLLQ_GLOBAL, N.OPT_ROLLQ_MERGE)),
                       ([L[LONG_N[0]], E["short"]], (0, N.OPT_ROLLQ_MERGE, N.OPT_ROLLQ_GLOBAL))):
        for opt in opts:
            for e, r in zip(envs, det.run_env_host(envs, SR, p, stages, options=opt)):
                _check(r, _answer(e, p), (e.size, w, opt))


@functools.lru_cache(maxsize=None)
def _many_trough_envelope():
    """More raw troughs at distance 2 than k_draft_bounds stages (DB_TRMAX)."""
    rng = np.random.default_rng(2040)
    return np.ascontiguousarray(rng.random(12000) * 10 + 5 * _beat(12000))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [151, 3020])
def test_draft_staging_limits(det, w):
    """Distance 2 on a rough envelope: more raw troughs than k_draft_bounds
    stages (DB_TRMAX) or ranks recording-wide (DB_LOCAL_M), and windows of far
    more than 64 trough segments (k_draft_points' [wide] launch)."""
    from bpm_analysis_amd import _native as N
    E = _window_envelopes()
    many = _many_trough_envelope()
    batch = [many, E["short"], E["many"]]
    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    for q, mult in ((0.2, 4.0), (0.5, 1.0), (0.0, 1.0)):
        p = _params(distance=2, window=w, noise_floor_quantile=q, trough_rejection_multiplier=mult)
        o = _answer(many, p)
        assert o["n_raw"] > DB_TRMAX > DB_LOCAL_M
        assert o["n_raw"] * w // many.size > 64 or w < 3020
        a = det.run_env_host(batch, SR, p, stages, options=N.OPT_STATS)
        undecided = det.stats()["undecided"]
        for e, r in zip(batch, a):
            _check(r, _answer(e, p), ("distance 2", e.size, w, q, mult))
        for opt in ROLLQ_VARIANTS:
            _check_equal_runs(a, det.run_env_host(batch, SR, p, stages, options=getattr(N, opt)),
                              ("distance 2", w, q, opt))
        if mult == 1.0 and q == 0.5:
            assert undecided > 0


# ----------------------------------------------------------------------------
# recordings beyond WM_MMAX and FPL_NMIN: the host's kernel selection
# ----------------------------------------------------------------------------
# The switch points are detect_plan's (csrc/bpmx_plan.h: cap, merge_g, wm_c); tests/test_plan.py
# reads them off the plan itself at the windows below.
LONG_N = [WM_MMAX + 64, 20000, 66000]
LONG_WINDOWS = [3, 151, 3841, 3842, 7937, 7938, 16385, 16386] + [n + 5 for n in LONG_N]
LONG_DISTANCES = [1, 15, 300]
LONG_OTHER = (151, 3842, 16386)              # these windows also at distances 1 and 300
LONG_MID = (3842, 7938, 16386, 20005)        # and these on a batch without a recording past FPL_NMIN


@pytest.mark.gpu
@pytest.mark.parametrize("w", [3842, 7937])
def test_union_kernel_edge_words_beyond_64(det, w):
    """Regression: k_rolling_quantile<RQ_T,32> (windows of 3842 to 7937
    samples) holds up to 8192 union members, 128 words of edge bits, but
    scanned the first 64 words' counts only, so edge entries of higher sorted
    indices overwrote the start of the edge list.  First seen on the
    sparse-then-dense 66000-sample envelope at W = 3842, distance 300 (its
    window's largest value an edge sample); at W = 7937 and level 0.9 nearly
    every window walks such edges.  BPMX_OPT_ROLLQ_MERGE sends the short
    recordings there as well."""
    from bpm_analysis_amd import _native as N
    assert 16 * RQ_T < _cap(w) <= 32 * RQ_T
    E, L = _window_envelopes(), _long_envelopes()
    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    for k, q in ((300, 0.2), (15, 0.9)):
        p = _params(distance=k, window=w, noise_floor_quantile=q)
        envs = [L["sparse_dense"], E["beat"], E["rough"]]
        for opt in (0, N.OPT_ROLLQ_MERGE):
            for e, r in zip(envs, det.run_env_host(envs, SR, p, stages, options=opt)):
                _check(r, _answer(e, p), (e.size, w, k, q, opt))


def _cap(w):
    return (w + RQ_T - 1 + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _long_envelopes():
    rng = np.random.default_rng(66000)
    out = {}
    for n in LONG_N + [5000]:
        t = np.arange(n)
        out[n] = 200 + 80 * np.sin(t / 700.0) + 300 * _beat(n) + rng.random(n)
    out["pairs"] = _spike_pairs(LONG_DISTANCES, 8)
    # sparse maxima (k_fpl_dist_ch cuts them into chunks at gaps >= distance),
    # then dense noise: one component past the chunk halo
    out["sparse_dense"] = np.concatenate([300 * _beat(33000, 700.0) + 20, rng.random(33000) * 10 + 5])
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in out.items()}


def test_long_recording_grid_is_on_the_switches():
    """The windows of test_long_recording_param_boundaries sit on both sides
    of each switch of the host's selection, and its distances are sensitive."""
    E = _long_envelopes()
    assert LONG_N[0] > WM_MMAX and LONG_N[0] - 64 <= WM_MMAX and LONG_N[2] > FPL_NMIN
    assert _cap(3841) == 16 * RQ_T < _cap(3842) and _cap(7937) == 32 * RQ_T < _cap(7938)
    assert (WM_MMAX - 16385 + 1) // 64 * 64 == 2048 > (WM_MMAX - 16386 + 1) // 64 * 64
    small = [E["pairs"], E[5000]]
    _assert_sensitive(small, LONG_DISTANCES, lambda k: _params(distance=k), lowest=1, same=_same_distance(20000))
    # the halo hand-over: sparse beats (gaps >= 300 between maxima), then > 1024 maxima without such a gap
    sd = E["sparse_dense"]
    cand = O.find_peaks(sd)
    gaps = np.diff(cand)
    assert (gaps[cand[1:] < 33000] >= 300).all() and (gaps[cand[:-1] >= 33000] < 300).all()
    assert (cand >= 33000).sum() > 2 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("w", LONG_WINDOWS)
def test_long_recording_param_boundaries(det, w):
    """Recordings just past WM_MMAX and past FPL_NMIN with a short one in the
    batch, noise windows on both sides of each switch in the host's rolling-
    quantile selection (<RQ_T,16> / <RQ_T,32> / the global union; chunked
    wavelet matrix or not), distances 1 / 15 / 300 through the k_fpl_* kernels
    (with sparse beats before dense noise for k_fpl_dist_ch's halo at 300),
    default and BPMX_OPT_ROLLQ_MERGE; at three of the windows also the
    noise-floor levels 0, 0.999 and 1."""
    from bpm_analysis_amd import _native as N
    E = _long_envelopes()
    # the cheap envelopes first: the oracle runs until one differs
    _assert_sensitive([E[5000], E[LONG_N[0]], E[20000], E[66000]], [w], lambda w: _params(window=w), lowest=3,
                      same=_same_window(66000))
    stages = N.STAGE_FLOOR | N.STAGE_PEAKS
    batch = [E[LONG_N[0]], E[66000], E[5000], E[20000], E["pairs"]]
    mid = [E[LONG_N[0]], E[5000], E[20000]]               # k_find_peaks_lds for all
    for k in LONG_DISTANCES if w in LONG_OTHER else (15,):
        p = _params(distance=k, window=w)
        envs = batch + ([E["sparse_dense"]] if k == 300 else [])
        for opt in (0, N.OPT_ROLLQ_MERGE):
            a = det.run_env_host(envs, SR, p, stages, options=opt)
            for e, r in zip(envs, a):
                _check(r, _answer(e, p), (e.size, w, k, opt))
        if k == 15 and w in LONG_MID:
            a = det.run_env_host(mid, SR, p, stages)
            for e, r in zip(mid, a):
                _check(r, _answer(e, p), ("mid", e.size, w, k))
        if k == 15 and w in LONG_OTHER:                   # the levels' ends through the long recordings' kernels
            for q in (0.0, 0.999, 1.0):
                pq = _params(window=w, noise_floor_quantile=q)
                for opt in (0, N.OPT_ROLLQ_MERGE):
                    for e, r in zip(mid, det.run_env_host(mid, SR, pq, stages, options=opt)):
                        _check(r, _answer(e, pq), ("mid", e.size, w, q, opt))


# ----------------------------------------------------------------------------
# the quantile levels' slots
# ----------------------------------------------------------------------------
# (trough_prominence_quantile, peak_prominence_quantile, noise_floor_quantile);
# the all-NaN fallback's level is always 0.1
LEVEL_PATTERNS = {
    "distinct": (0.15, 0.25, 0.3),
    "noise_is_trough": (0.15, 0.25, 0.15),
    "noise_is_peak": (0.15, 0.25, 0.25),
    "noise_is_fallback": (0.15, 0.25, 0.1),
    "all_equal": (0.1, 0.1, 0.1),
    "default": (0.1, 0.1, 0.2),
}


def _level_params(pattern):
    qt, qp, qn = LEVEL_PATTERNS[pattern]
    return dict(G.BASE_PARAMS, trough_prominence_quantile=qt, peak_prominence_quantile=qp, noise_floor_quantile=qn)


@pytest.mark.gpu
def test_quantile_level_sharing(det):
    """The levels deduplicated into slots (one radix select per distinct
    level), the noise level lazy unless it equals another: every sharing
    pattern at env level (FLOOR alone and FLOOR | PEAKS, with a recording of
    fewer than 5 troughs, whose static floor is the noise level itself) and in
    native mode, where k_hilbert_env selects all of them from the envelope it
    writes.  Native outputs are compared with the oracle's env-level functions
    on the GPU's own envelope, so bit for bit."""
    from bpm_analysis_amd import _native as N
    rng = np.random.default_rng(4)
    t = np.arange(7000)
    envs = [300 * _beat(5000) + rng.random(5000) + 20,
            rng.random(6000) ** 3 * 1000 + 50 * _beat(6000),
            _vshape([0, 500, 1100, 1800, 2300, 2999], [15.0, 950.0, 45.0, 1010.0, 25.0, 820.0], 3000),
            200 + 80 * np.sin(t / 700.0) + 300 * _beat(7000) + rng.random(7000)]
    static = 0
    for pattern in LEVEL_PATTERNS:
        p = _level_params(pattern)
        both = det.run_env_host(envs, SR, p, N.STAGE_FLOOR | N.STAGE_PEAKS)
        floor = det.run_env_host(envs, SR, p, N.STAGE_FLOOR)
        for e, r, rf in zip(envs, both, floor):
            o = _answer(e, p)
            _check(r, o, (pattern, e.size))
            _check(rf, o, (pattern, e.size, "FLOOR alone"), peaks=False)
            static += o["flags"] & 1
        o = _answer(envs[2], p)
        assert o["flags"] & 1 and np.all(o["floor"] == np.quantile(envs[2], p["noise_floor_quantile"]))
    assert static == len(LEVEL_PATTERNS)

    # native mode, short int16 recordings whose Nd the fused Hilbert kernel plans
    fs, ds = 44100, 146
    nds = [2406, 1000, 18]
    recs = [O.synth(800 + i, nd * ds - i, fs, 1) for i, nd in enumerate(nds)]
    want_env = None
    det.profile_only("")
    for pattern in LEVEL_PATTERNS:
        p = _level_params(pattern)
        det.profile(True)
        res = det.run_host(recs, fs, p, mode="native", want_y=False)
        det.profile(False)
        assert "k_quantile_reg" not in det.profile_read()      # every level came from k_hilbert_env
        if want_env is None:
            want_env = [O.detect(pcm, fs, p, mode="native")["env"] for pcm in recs]
        for nd, r, we in zip(nds, res, want_env):
            assert r["env"].size == nd and r["sr"] == SR
            assert np.max(np.abs(r["env"] - we)) <= 1e-9 * np.max(np.abs(we))
            env = np.ascontiguousarray(r["env"])
            o = _answer(env, p, sr_fs=fs)
            _check(r, o, (pattern, nd, "native"))
            if nd == 18:
                assert o["flags"] & 1
