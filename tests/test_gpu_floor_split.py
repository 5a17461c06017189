"""The floor after the draft as two half-recording workgroups per recording
(k_floor_wm_half, the default when the longest recording is eligible by
length) against the one-workgroup launch (BPMX_OPT_FLOOR_ONEWG) and the
oracle, bit for bit: floor, troughs and flags.

Envelopes go straight in at 302 Hz.  Most cases use a noise window of 1-2 s
(W = 302 .. 604 samples), so that a recording is eligible from 2 W + 128
samples on and the cases stay at 1-3 K samples; the cap and table cases need
the flagship length (18124 samples), where a half reaches more than
WMH_PMAX = 4224 samples."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import goldens as G

pytestmark = pytest.mark.gpu

SR = 302
FLAG_MASK = 3 | 4 | O.F_TROUGH_TIE          # static / draft / all-NaN fallbacks, decisive trough ties
WM_MMAX, WM_TRMAX, WMH_PMAX = 18432, 512, 4224


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _params(window_sec=1.0, **kw):
    return dict(G.BASE_PARAMS, noise_window_sec=window_sec, **kw)


def _beat(n, period=80.0):
    return np.maximum(0.0, np.sin(2 * np.pi * np.arange(n) / period)) ** 8


def _plain(n, seed, period=80.0):
    return 300 * _beat(n, period) + np.random.default_rng(seed).random(n) + 20


def _split(n):
    """The boundary between the halves: n / 2 rounded up to a multiple of 64."""
    return ((n + 1) // 2 + 63) // 64 * 64


def _oracle(env, params):
    of, ot, ofl = O.noise_floor(env, O.derive(SR, params), params)
    return of, ot, ofl


def _run3(det, envs, params, want_split=True):
    """Default, one-workgroup and oracle results of one batch, compared
    pairwise; returns the default run's fallback count and launch labels."""
    from bpm_analysis_amd import _native as N
    det.profile_only("")
    det.profile(True)
    a = det.run_env_host(envs, SR, params, N.STAGE_FLOOR, options=N.OPT_STATS)
    det.profile(False)
    prof = det.profile_read()
    redo = det.floor_whole()
    b = det.run_env_host(envs, SR, params, N.STAGE_FLOOR, options=N.OPT_FLOOR_ONEWG)
    for i, (env, x, y) in enumerate(zip(envs, a, b)):
        of, ot, ofl = _oracle(env, params)
        for k, w in (("floor", of), ("troughs", ot)):
            assert _same(x[k], y[k]), (i, env.size, k, "split vs one workgroup")
            assert _same(x[k], w), (i, env.size, k, "split vs oracle")
        assert x["flags"] == y["flags"], (i, env.size)
        assert (x["flags"] & FLAG_MASK) == (ofl & FLAG_MASK), (i, env.size)
    assert ("k_floor_wm" in prof) == (want_split is not None)      # None: a long recording, no k_floor_wm at all
    assert ("k_floor_wm[whole]" in prof) == bool(want_split)
    return redo, prof


def test_eligibility_threshold(det):
    """n = 2 W + 128 takes the one-workgroup launch, n = 2 W + 129 the split
    one, without a fallback."""
    from bpm_analysis_amd import _native as N
    p = _params(1.0)
    W = O.derive(SR, p).noise_window
    assert W == 302
    redo, _ = _run3(det, [_plain(2 * W + 128, 1)], p, want_split=False)
    assert redo == 0
    redo, prof = _run3(det, [_plain(2 * W + 129, 2)], p, want_split=True)
    assert redo == 0
    # the option forces the old launch
    det.profile(True)
    det.run_env_host([_plain(2 * W + 129, 2)], SR, p, N.STAGE_FLOOR, options=N.OPT_FLOOR_ONEWG)
    det.profile(False)
    assert "k_floor_wm[whole]" not in det.profile_read()


@pytest.mark.parametrize("window_sec", [1.0, 1.5])            # W = 302 (even), 453 (odd)
def test_boundary_and_partial_blocks(det, window_sec):
    """n mod 64 in {0, 1, 63} and an odd n: the boundary h and the last block
    of each half are partial; each recording alone and all in one batch."""
    p = _params(window_sec)
    assert O.derive(SR, p).noise_window % 2 == (0 if window_sec == 1.0 else 1)
    ns = [1536, 1537, 1599, 2001, 1089]                       # mod 64: 0, 1, 63, 17 (odd), 1 (h = 576 > n / 2)
    assert [n % 64 for n in ns] == [0, 1, 63, 17, 1]
    envs = [_plain(n, 10 + i) for i, n in enumerate(ns)]
    for e in envs:
        redo, _ = _run3(det, [e], p)
        assert redo == 0
    redo, _ = _run3(det, envs, p)
    assert redo == 0


def _late_first(n, start):
    """No trough before `start`: a steep fall there, beats after it."""
    e = _plain(n, 31)
    e[:start] = e[start] + 400.0 + 5.0 * np.arange(start, 0, -1)
    return e


def _early_last(n, stop):
    """No trough after `stop`: beats, then a steep rise to the end."""
    e = _plain(n, 32)
    e[stop:] = e[stop - 1] + 400.0 + 5.0 * np.arange(1, n - stop + 1)
    return e


def test_half_without_valid_output_falls_back(det):
    """First trough beyond h + W / 2: half 0 has no valid output, the bfill
    crosses the boundary, and the recording is recomputed whole.  The mirror
    image, last trough before h - W / 2: np.interp holds the last trough's
    value to the end of the recording, so half 1 still has 3 or more
    observations in every window, has valid outputs of its own and no ffill
    crosses the boundary; the halves finish it, and the floor past the last
    trough equals the oracle's.  A first trough inside half 0: its NaN prefix
    is filled by half 0 alone."""
    p = _params(1.0)
    W, n = 302, 2600
    h = _split(n)
    late = _late_first(n, h + W)
    _, tr, _ = _oracle(late, p)
    assert tr.size > 2 and tr[0] > h + W // 2
    redo, _ = _run3(det, [late], p)
    assert redo == 1
    early = _early_last(n, h - W)
    _, tr, _ = _oracle(early, p)
    assert tr.size > 2 and tr[-1] < h - W // 2
    redo, _ = _run3(det, [early], p)
    assert redo == 0
    mid = _late_first(n, h // 2)
    of, tr, _ = _oracle(mid, p)
    assert h // 2 <= tr[0] < h
    redo, _ = _run3(det, [mid], p)
    assert redo == 0


def _stress(n=18124):
    """Flagship-length envelopes in the style of the pruning stress set."""
    rng = np.random.default_rng(7)
    t = np.arange(n)
    beat = np.maximum(0.0, np.sin(2 * np.pi * t / 250.0)) ** 8
    h = _split(n)
    ulp = 10.0 + np.spacing(10.0) * rng.integers(0, 5, n) + 300 * beat
    return {
        "ulp": ulp,                                                            # every sample kept: both halves overflow
        "ulp_half0": np.where(t < h, ulp, 200 + 0.01 * t + 300 * beat + rng.random(n)),   # only half 0 overflows
        "ulp_half1": np.where(t >= h, ulp, 200 + 0.01 * t + 300 * beat + rng.random(n)),  # only half 1 overflows
        "ramp": 10.0 + 0.05 * t + 3000 * beat + rng.random(n),
        "rough": rng.random(n) ** 3 * 1000 + 50 * beat,
        "troughs>512": np.abs(np.sin(t / 9.0)) * 100 + rng.random(n),
        "wander": 200 + 80 * np.sin(t / 700.0) + 300 * beat + rng.random(n),
    }


@pytest.mark.parametrize("window_sec", [1.0, 10])
def test_cap_and_trough_table(det, window_sec):
    """Ulp-level plateaus keep every sample, so a half's kept set exceeds
    WMH_PMAX in both halves, in half 0 only, in half 1 only; more than
    WM_TRMAX sanitised troughs: all handed back.  Of the ramp, the rough and
    the slow-wander envelopes, tools/prune_sim.py's half_kept puts all three
    above the cap at the 1 s window (86-100 % kept) and only the ramp at the
    10 s one (8043 / 9024 kept; rough 2613 / 3844, wander 3438 / 3353)."""
    p = _params(window_sec)
    s = _stress()
    _, tr, _ = _oracle(s["troughs>512"], p)
    assert tr.size > WM_TRMAX
    for name in ("ulp", "ulp_half0", "ulp_half1", "troughs>512"):
        redo, _ = _run3(det, [s[name]], p)
        assert redo == 1, name
    names = list(s)
    redo, _ = _run3(det, [s[k] for k in names], p)
    assert redo == (7 if window_sec == 1.0 else 5)


def _vshape(pos, val, n):
    return np.interp(np.arange(n), pos, val)


def _other_routes():
    few = _vshape([0, 500, 1100, 1800, 2300, 2999], [15.0, 950.0, 45.0, 1010.0, 25.0, 820.0], 3000)   # < 5 raw troughs
    return [few, _plain(2400, 41)]


def test_other_routes(det):
    """Fewer than 5 raw troughs (the static floor), 2 or fewer sanitised
    troughs (the draft floor: a rejection multiplier that rejects all): each
    is handed back whole.  A floor that is NaN everywhere is not among the
    cases: it needs a first trough within 2 samples of the end, which 3 kept
    troughs at find_peaks' distance rule out for a finite envelope, and on an
    envelope with -inf troughs the one-workgroup launch itself gives NaN where
    the oracle gives -inf (both launches agree there; the halves hand a
    non-finite curve back)."""
    p = _params(1.0)
    few, plain = _other_routes()
    _, _, fl = _oracle(few, p)
    assert fl & 1
    redo, _ = _run3(det, [few], p)
    assert redo == 1
    p0 = _params(1.0, trough_rejection_multiplier=0.0)
    _, tr, fl = _oracle(plain, p0)
    assert fl & 2 and tr.size <= 2
    redo, _ = _run3(det, [plain], p0)
    assert redo == 1


def test_ragged_batch(det):
    """Everything above in one ragged batch: eligible, too short, late first
    trough, few troughs, capped; then the same with a recording longer than
    WM_MMAX, which sends the whole run down the long-recording route."""
    p = _params(1.0)
    W, n = 302, 2600
    h = _split(n)
    s = _stress()
    few, plain = _other_routes()
    envs = [_plain(1537, 50), _plain(2 * W + 128, 51), _plain(300, 52), _late_first(n, h + W), _early_last(n, h - W),
            few, plain, s["ulp_half0"], s["troughs>512"], s["wander"], _plain(1599, 53)]
    redo, _ = _run3(det, envs, p)
    # too short x2, late first trough, few troughs, cap x2 (at this window the slow wander keeps 97 % of its
    # samples, tools/prune_sim.py's half_kept), > 512 troughs
    assert redo == 7
    long_ = _plain(WM_MMAX + 700, 54)
    _run3(det, envs + [long_], p, want_split=None)


def test_flagship_has_no_fallback(det):
    """The first 16 bench recordings (det.synth seeds 0..15, 60 s at 44.1 kHz,
    default parameters, native mode): no recording is handed back, and the
    one-workgroup launch gives the same bits."""
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd.config import DEFAULT_PARAMS
    fs, nfr, F = 44100, 2646000, 16
    fo = np.arange(F + 1, dtype=np.int64) * nfr
    params = dict(DEFAULT_PARAMS)
    pcm = det.synth(fo, fs, 1, seed0=0)
    det.profile_only("")
    det.profile(True)
    a = det.run(pcm, fo, fs, params, mode="native", options=N.OPT_STATS).to_host()
    det.profile(False)
    assert "k_floor_wm[whole]" in det.profile_read()
    assert det.floor_whole() == 0
    b = det.run(pcm, fo, fs, params, mode="native", options=N.OPT_FLOOR_ONEWG).to_host()
    for x, y in zip(a, b):
        for k in ("floor", "troughs", "peaks"):
            assert _same(x[k], y[k]), k
        assert x["flags"] == y["flags"]
