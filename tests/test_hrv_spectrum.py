"""``hrv_spectrum.spectrum_ints`` (the definition of bpmx_hrvspec_device in
numpy) against ``scipy.signal.lombscargle(..., normalize=True,
floating_mean=True)`` on every valid window of the shared cases, within the
derived bound of tests/hrvspec_cases.py; the band values and decisions, the
window count, the geometry and the CSV round trip.

The oracle is called on the centred ``u``, not on ``y``: on raw intervals near
1000 ms scipy's own floating-mean subtraction loses (mean / sigma)^2."""
import math

import numpy as np
import pytest
from scipy.signal import lombscargle

from bpm_analysis_amd import hrv_spectrum as HS
from tests import hrvspec_cases as HC


def _windows(c):
    """(w, s, u, S) of every window of the case, from the definition's text alone."""
    g, idx = c["g"], c["idx"]
    if not c["ok"] or len(idx) < 2:
        return
    d, e = np.diff(idx), idx[1:]
    keep = (d >= g["dmin"]) & (d <= g["dmax"])
    d, e = d[keep], e[keep]
    for w in range(HS.n_windows(c["nd"], g["win"], g["hop"])):
        sel = (e >= w * g["hop"]) & (e < w * g["hop"] + g["win"])
        y = d[sel] * 1000.0 / c["sr"]
        yield w, (e[sel] - e[sel][0] if sel.any() else e[sel]).astype(np.float64), y, e[sel]


def test_q_is_scipys_lombscargle_within_the_bound():
    worst, n_valid = 0.0, 0
    for c, want in zip(HC.cases(), HC.expected()):
        om = HS.omegas(c["g"])
        for w, s, y, e in _windows(c):
            assert want["n_rr"][w] == len(y), (c["name"], w)
            if want["code"][w] != 0:
                assert np.isnan(want["q"][w]).all()
                continue
            n_valid += 1
            u = y - y.sum() / len(y)
            ref = lombscargle(s, u, om, normalize=True, floating_mean=True)
            share = np.abs(np.atleast_1d(ref) - want["q"][w]) / want["tol"][w]
            worst = max(worst, float(share.max()))
            assert (share <= 1.0).all(), (c["name"], w, float(share.max()))
            assert want["var"][w] == pytest.approx(float(np.mean(u * u)), rel=1e-14)
            assert want["time"][w] == float(e[0] + e[-1]) / (2.0 * c["sr"])
    assert n_valid > 150
    print(f"largest share of the bound used against scipy: {worst:.2e}")


def test_codes_counts_and_bands():
    by = {c["name"]: (c, w) for c, w in zip(HC.cases(), HC.expected())}
    for name, (c, w) in by.items():                                     # no peak decision of the cases is open
        assert HC.open_peaks(w) == [], name
        assert len(w["code"]) == HS.n_windows(c["nd"], c["g"]["win"], c["g"]["hop"])
    assert "golden_vulpine" in by and len(by["golden_vulpine"][1]["code"]) == 9
    assert (by["few"][1]["code"] == 1).all() and (by["short_span"][1]["code"] == 2).all()
    assert (by["constant"][1]["code"] == 3).all() and by["constant"][1]["n_rr"].min() >= 8
    w = by["all_excluded"][1]
    assert (w["code"] == 1).all() and (w["n_rr"] == 0).all() and np.isnan(w["time"]).all()
    assert set(by["excluded_then_rhythm"][1]["code"]) == {0, 1, 2}
    assert by["min_intervals_exact"][1]["n_rr"][0] == 8 and by["min_intervals_exact"][1]["code"][0] == 0
    assert by["min_intervals_less"][1]["n_rr"][0] == 7 and by["min_intervals_less"][1]["code"][0] == 1
    assert by["span_exact"][1]["code"][0] == 0 and by["span_less"][1]["code"][0] == 2
    c, w = by["interval_edges"]
    d = np.diff(c["idx"])
    assert {24, 25, 150, 151} <= set(d.tolist())
    assert w["n_rr"].sum() > 0 and (w["code"] == 0).all()
    e = c["idx"][1:]
    in0 = (e >= 0) & (e < c["g"]["win"])
    assert w["n_rr"][0] == int((in0 & (d >= 25) & (d <= 150)).sum()) < int(in0.sum())
    assert [len(by[f"nd_{n}"][1]["code"]) for n in (0, 2999, 3000, 3001, 3749, 3750)] == [0, 1, 1, 1, 1, 2]
    for nq in (1, 256, 300):
        w = by[f"n_freq_{nq}"][1]
        assert w["q"].shape[1] == nq and (w["code"] == 0).all()
        assert ((w["q"] >= 0) & (w["q"] <= 1 + 1e-12)).all()
    w = by["n_freq_1"][1]
    assert (w["lf_peak"] == 0).all() and (w["hf_peak"] == -1).all() and (w["hf"] == 0.0).all()
    w = by["lf_empty_hf_all"][1]
    assert (w["lf"] == 0.0).all() and (w["lf_peak"] == -1).all() and (w["hf"] > 0).all()
    assert w["record"][3] == 0.0 and w["record"][4] == 0.0 and w["record"][0] == 5
    w = by["hf_empty_at_end"][1]
    assert (w["hf"] == 0.0).all() and (w["hf_peak"] == -1).all() and np.isnan(w["record"][3]) and w["record"][4] == 1.0
    w = by["one_point_bands"][1]
    assert (w["lf_peak"] == 0).all() and (w["hf_peak"] == 36).all()
    for n in (0, 1):
        w = by[f"n_final_{n}"][1]
        assert w["status"] == HS.NONE and (w["code"] == 1).all() and (w["n_rr"] == 0).all() and w["record"][0] == 0
    assert by["n_final_2"][1]["status"] == HS.OK and by["n_final_2"][1]["n_rr"].max() == 1
    w = by["bad_status"][1]
    assert w["status"] == HS.NONE and len(w["code"]) == 14 and np.isnan(w["record"][1:]).all()
    w = by["rhythm"][1]                                                 # the respiratory line at 0.25 Hz is the HF peak
    hz = HS.peak_hz(w, w["hf_peak"])
    assert np.all(np.abs(hz - 0.25) < 0.03) and (w["hf"] > w["lf"]).all()
    rec = w["record"]
    assert rec[0] == 14 and rec[1] == pytest.approx(w["lf"].mean()) and rec[3] == pytest.approx((w["lf"] / w["hf"]).mean())
    assert rec[4] == pytest.approx((w["lf"] / (w["lf"] + w["hf"])).mean()) and np.isnan(rec[5:]).all()


def test_geometry_and_window_count():
    g = HS.geometry(302)
    assert (g["win"], g["hop"], g["dmin"], g["dmax"], g["min_intervals"], g["n_freq"]) == (36240, 9060, 76, 453, 16, 256)
    from bpm_analysis_amd import tempo as TP
    assert (g["dmin"], g["dmax"]) == TP.geometry(302)[2:]
    assert g["min_span"] == math.ceil(302 / 0.04) and (g["lf_a"], g["hf_b"]) == (0, 256) and g["lf_b"] == g["hf_a"] == 78
    f = HS.omegas(g) * 302 / (2 * math.pi)
    assert f[0] == pytest.approx(0.04) and f[-1] == pytest.approx(0.40) and f[77] < 0.15 <= f[78] + 1e-12
    assert g["scale"] == pytest.approx((f[1] - f[0]) / 302)
    g = HS.geometry(1000, dict(min_bpm=120, max_bpm=600), win_sec=30, hop_sec=5, n_freq=64, f_lo=0.5, f_hi=3.0,
                    lf_band=(0.5, 1.0), hf_band=(1.0, 3.0))           # an animal that breathes faster
    assert (g["dmin"], g["dmax"], g["win"], g["hop"], g["min_span"]) == (100, 500, 30000, 5000, 2000)
    assert g["lf_a"] == 0 and g["lf_b"] == g["hf_a"] and g["hf_b"] == 64
    HS.check_geometry(g)
    for bad in (dict(hop=0), dict(dmin=0), dict(dmax=75), dict(min_intervals=2), dict(n_freq=0), dict(n_freq=1025),
                dict(lf_a=-1), dict(lf_b=257), dict(hf_a=200, hf_b=100), dict(om0=0.0), dict(dom=-1e-9),
                dict(om0=float("nan")), dict(dom=float("inf"))):
        with pytest.raises(ValueError):
            HS.check_geometry(dict(HS.geometry(302), **bad))
    assert [HS.n_windows(n, 10, 3) for n in (-1, 0, 1, 9, 10, 11, 12, 13, 16)] == [0, 0, 1, 1, 1, 1, 1, 2, 3]
    assert HS.n_windows(100, 0, 1) == 0 and HS.n_windows(100, 10, 0) == 0


def test_spectrum_is_spectrum_ints_at_the_geometry():
    c = HC.cases()[0]
    a, b = HS.spectrum(c["idx"], c["nd"], c["sr"]), HC.expected()[0]
    for k in ("code", "n_rr", "lf", "hf", "lf_peak", "hf_peak", "q", "record"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert "tol" not in a and "tol" in b


@pytest.mark.parametrize("name", ["wander1", "excluded_then_rhythm", "lf_empty_hf_all", "bad_status", "nd_0"])
def test_csv_round_trip(tmp_path, name):
    want = dict(zip((c["name"] for c in HC.cases()), HC.expected()))[name]
    path = HS.spectrum_path("/some/where/rec7.wav", str(tmp_path))
    assert path.endswith("rec7_hrv_spectrum.csv")
    HS.write_csv(path, want)
    got = HS.read_csv(path)
    for k in ("time", "lf", "hf"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k         # repr: the doubles as they were
    assert np.array_equal(got["n_rr"], want["n_rr"]) and np.array_equal(got["code"], want["code"])
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(got["lf_hf"], np.where(want["hf"] > 0, want["lf"] / want["hf"], np.nan), equal_nan=True)
    assert np.array_equal(got["lf_peak_hz"], HS.peak_hz(want, want["lf_peak"]), equal_nan=True)
    assert np.array_equal(got["hf_peak_hz"], HS.peak_hz(want, want["hf_peak"]), equal_nan=True)
    for k in HS.INT_KEYS + HS.FLOAT_KEYS + ("sr", "status"):
        assert got[k] == want[k], k
    assert np.array_equal(got["record"], want["record"], equal_nan=True)
    lines = open(path).read().splitlines()
    assert lines[0].startswith("Time (s),Intervals,Code,LF") and sum(ln.startswith("# ") for ln in lines) == 21
