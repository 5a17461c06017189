"""bpm_analysis_amd/tempo.py on the host: ``compare`` on hand-made curves,
``write_csv`` / ``read_csv`` round trips, and ``tempogram`` on the vulpine
golden against a recorded fixture of its own lag column
(tests/golden/vulpine_tempo_lag.txt), so the host statement of the stage cannot
drift silently."""
import os

import numpy as np
import pytest

from bpm_analysis_amd import tempo as TP
from tests import tempo_cases as TC

FIXTURE = os.path.join(TC.GOLDEN, "vulpine_tempo_lag.txt")


def _table(bpm, rho=None, min_strength=0.3):
    n = len(bpm)
    rho = np.full(n, 0.8) if rho is None else np.asarray(rho, float)
    return dict(time=4.0 + 2.0 * np.arange(n), lag=np.full(n, 100, np.int32), rho=rho, bpm=np.asarray(bpm, float),
                min_strength=min_strength)


def test_compare_on_hand_made_curves():
    t = _table([100.0, 110.0, 120.0, 130.0])
    times = np.array([0.0, 4.0, 6.0, 8.0, 10.0, 20.0])
    curve = np.array([90.0, 100.0, 110.0, 120.0, 130.0, 130.0])
    assert TP.compare(t, times, curve) == dict(n=4, agree=1.0, double=0.0, half=0.0, other=0.0, tol=0.1)
    assert TP.compare(t, times, 2 * curve) == dict(n=4, agree=0.0, double=1.0, half=0.0, other=0.0, tol=0.1)
    assert TP.compare(t, times, curve / 2) == dict(n=4, agree=0.0, double=0.0, half=1.0, other=0.0, tol=0.1)
    assert TP.compare(t, times, 1.5 * curve) == dict(n=4, agree=0.0, double=0.0, half=0.0, other=1.0, tol=0.1)
    # within the tolerance on either side, outside just beyond it; the curve is interpolated at the centres
    assert TP.compare(t, times, 1.09 * curve)["agree"] == 1.0 and TP.compare(t, times, 0.91 * curve)["agree"] == 1.0
    assert TP.compare(t, times, 1.11 * curve)["other"] == 1.0
    assert TP.compare(t, [0.0, 20.0], [100.0, 140.0], tol=0.11)["agree"] == 1.0        # 108, 112, 116, 120 there
    mixed = np.array([90.0, 100.0, 220.0, 60.0, 200.0, 200.0])
    assert TP.compare(t, times, mixed) == dict(n=4, agree=0.25, double=0.25, half=0.25, other=0.25, tol=0.1)
    # only strong windows count; a curve's NaN rows and order do not matter
    weak = _table([100.0, 110.0, 120.0, 130.0], rho=[0.8, 0.1, 0.8, 0.29])
    assert TP.compare(weak, times, mixed) == dict(n=2, agree=0.5, double=0.0, half=0.5, other=0.0, tol=0.1)
    shuffled = np.array([3, 0, 5, 1, 4, 2])
    withnan = (np.concatenate([times[shuffled], [7.0]]), np.concatenate([mixed[shuffled], [np.nan]]))
    assert TP.compare(weak, *withnan) == TP.compare(weak, times, mixed)


def test_compare_with_nothing_to_compare():
    t = _table([100.0, 110.0], rho=[0.1, 0.2])
    assert TP.compare(t, [0.0, 10.0], [100.0, 100.0]) is None                 # no strong window
    invalid = dict(_table([np.nan, np.nan]), lag=np.zeros(2, np.int32), rho=np.zeros(2))
    assert TP.compare(invalid, [0.0, 10.0], [100.0, 100.0]) is None
    assert TP.compare(_table([100.0]), [], []) is None                        # no curve
    assert TP.compare(_table([]), [0.0], [100.0]) is None                     # no window


@pytest.mark.parametrize("name", ["weak_then_strong", "one_nan", "nd_95", "golden_ref_44k_10s_zeros"])
def test_write_csv_round_trips(tmp_path, name):
    want = dict(TC.expected()[[c["name"] for c in TC.cases()].index(name)])
    chk = TP.compare(want, want["time"], want["bpm"] * 2) if name == "weak_then_strong" else None
    path = TP.tempo_path("/somewhere/else/rec 01.wav", str(tmp_path))
    assert path == str(tmp_path / "rec 01_tempo.csv")
    TP.write_csv(path, want, chk)
    got, got_chk = TP.read_csv(path)
    for k in ("time", "lag", "rho", "bpm"):
        assert np.array_equal(got[k], want[k], equal_nan=True) and got[k].dtype == want[k].dtype, k
    for k in ("sr", "win", "hop", "kmin", "kmax", "min_strength", "start_windows", "n_valid", "n_strong"):
        assert got[k] == want[k] and type(got[k]) is type(want[k]), k
    for k in ("median_bpm", "mean_rho", "hint"):
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
    assert got_chk == chk
    if chk is not None:
        assert chk["double"] == 1.0
    head = open(path).readline().strip()
    assert head == "Time (s),Lag (samples),Strength,BPM"


def test_geometry_and_window_count():
    assert TP.geometry(302) == (2416, 604, 76, 453)
    assert TP.geometry(147) == (1176, 294, 37, 220)
    assert TP.geometry(1000, dict(min_bpm=30, max_bpm=300)) == (8000, 2000, 200, 2000)
    assert TP.geometry(302, None, 4.0, 0.5) == (1208, 151, 76, 453)
    assert [TP.n_windows(n, 2416, 604) for n in (0, 2415, 2416, 3019, 3020, 18124)] == [0, 0, 1, 1, 2, 27]
    for bad in ((2416, 0, 76, 453), (2416, 604, 1, 453), (2416, 604, 76, 2415), (2416, 604, 454, 453)):
        with pytest.raises(ValueError):
            TP.tempogram_ints(np.ones(5000), 302, *bad)


def test_tempogram_on_vulpine_keeps_its_recorded_lags():
    env, sr = TC.golden_env("vulpine")
    d = TP.tempogram(env, sr)
    assert len(d["lag"]) == 185 and d["n_valid"] == 185 and (d["lag"] != 0).all()
    assert np.array_equal(d["lag"], np.loadtxt(FIXTURE, dtype=np.int32))
    assert d["lag"].min() >= 76 and d["lag"].max() <= 453
    assert np.array_equal(d["time"], (np.arange(185) * 604 + 1208) / 302)
    # what the definition was tried on: the first window says 98 BPM, and that is the hint
    assert round(d["bpm"][0]) == 98 and d["hint"] == d["bpm"][0] and d["rho"][0] >= 0.3
    strong = d["rho"] >= 0.3
    assert d["n_strong"] == strong.sum() and d["median_bpm"] == np.median(d["bpm"][strong])
    assert d["mean_rho"] == np.mean(d["rho"])
    # the parabola moves a lag by at most half a sample
    assert np.all(np.abs(60.0 * sr / d["bpm"] - d["lag"]) <= 0.5)


def test_tempogram_is_its_own_definition_written_out():
    """The vectorised sums against the loops of the definition's text, on a small case."""
    c = TC.cases()[[c["name"] for c in TC.cases()].index("weak_then_strong")]
    d = TP.tempogram_ints(c["env"], c["sr"], c["win"], c["hop"], c["kmin"], c["kmax"], c["min_strength"])
    x, win, hop, kmin, kmax = c["env"], c["win"], c["hop"], c["kmin"], c["kmax"]
    for w in range(len(d["lag"])):
        seg = x[w * hop:w * hop + win]
        m = sum(seg) / win
        e = [v - m for v in seg] + [0.0] * (kmax + 1)
        r = {k: sum(e[i] * e[i + k] for i in range(win)) for k in [0] + list(range(kmin - 1, kmax + 2))}
        cand = [k for k in range(kmin, kmax + 1) if r[k] > r[k - 1] and r[k] >= r[k + 1]]
        k = max(cand, key=lambda k: (r[k], -k))
        assert k == d["lag"][w]
        assert abs(r[k] / r[0] - d["rho"][w]) <= 1e-12
        delta = 0.5 * (r[k - 1] - r[k + 1]) / (r[k - 1] - 2 * r[k] + r[k + 1])
        assert abs(60.0 * c["sr"] / (k + delta) / d["bpm"][w] - 1) <= 1e-9
