"""Shared by test_metrics_core.py (CPU) and test_gpu_metrics.py: crafted beat
lists and curves for the final metrics, ``beats.final_metrics`` brought into
the form bpmx_metrics_core.h reports (curve positions, counts, doubles), the
comparison, and the binary exchange with metrics_core_driver."""
from __future__ import annotations

import contextlib
import datetime
import struct

import numpy as np
import pandas as pd

from bpm_analysis_amd import DEFAULT_PARAMS
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from tests import test_beats as TB

SR = 302
PARAMS = dict(DEFAULT_PARAMS, save_filtered_wav=False)
HRV_COLS = ("time", "rmssdc", "sdnn", "bpm")
RUN_COLS = ("a", "b", "slope", "dur")


@contextlib.contextmanager
def epoch(off_s=0):
    """``beats._EPOCH`` as on a machine `off_s` seconds east of UTC."""
    old = B._EPOCH
    B._EPOCH = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=off_s)
    try:
        yield
    finally:
        B._EPOCH = old


def case(fin, sr=SR, params=None, epoch_s=0, bst=0, curve=None):
    """One input of the core: final beats (samples) and their curve.  `curve`
    = (bpm_t, bpm) replaces the curve of the beats (the tie inputs); `bst` is
    the beats status the kernel would read."""
    params = params or PARAMS
    fin = np.ascontiguousarray(fin, np.int32)
    custom = curve is not None
    if curve is None:
        with epoch(epoch_s):
            s, t = B.bpm_series(fin.astype(np.int64), sr, params)
        curve = (np.asarray(t, np.float64), np.asarray(s.values, np.float64))
    bt, bv = (np.ascontiguousarray(a, np.float64) for a in curve)
    assert len(bt) == len(bv) and (len(bt) == 0 or len(bt) < len(fin))
    return dict(fin=fin, sr=int(sr), params=params, epoch_s=int(epoch_s), bst=int(bst), bt=bt, bv=bv, custom=custom)


def beats_of(rr_sec, sr=SR, t0=0.5):
    """Beat samples with the given RR intervals (seconds)."""
    t = t0 + np.concatenate([[0.0], np.cumsum(np.asarray(rr_sec, np.float64))])
    idx = np.round(t * sr).astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    return idx


def wander(n, seed, lo=55.0, hi=150.0, period=70.0, noise=0.04):
    """RR intervals of a heart rate that swings between lo and hi BPM."""
    rng = np.random.default_rng(seed)
    rr, t = [], 0.0
    for _ in range(n):
        bpm = (lo + hi) / 2 + (hi - lo) / 2 * np.sin(2 * np.pi * t / period + seed)
        r = 60.0 / bpm * (1 + noise * rng.standard_normal())
        rr.append(r)
        t += r
    return np.array(rr)


# ---- the reference side ------------------------------------------------------ #
def _pos(s, ts):
    ns = s.index.asi8
    v = pd.Timestamp(ts).value
    p = int(np.searchsorted(ns, v))
    assert ns[p] == v and (p + 1 == len(ns) or ns[p + 1] != v)
    return p


def _runs(s, runs, rising):
    a = np.array([_pos(s, r["start_time"]) for r in runs], np.int32)
    b = np.array([_pos(s, r["end_time"]) for r in runs], np.int32)
    for r, i, j in zip(runs, a, b):
        assert r["start_bpm"] == s.values[i] and r["end_bpm"] == s.values[j]
        ch = r["bpm_increase" if rising else "bpm_decrease"]
        assert ch == (s.values[j] - s.values[i] if rising else s.values[i] - s.values[j])
    return dict(a=a, b=b, slope=np.array([r["slope_bpm_per_sec"] for r in runs], np.float64),
                dur=np.array([r["duration_sec"] for r in runs], np.float64))


def normal_form(m):
    """A ``final_metrics`` dict as the device reports it.  ``inc`` / ``dec``
    None: find_peaks raised (the distance)."""
    s = m["smoothed_bpm"]
    rec = np.full(N.METRICS_RECORD, np.nan)
    for k, i in (("avg_bpm", N.MR_AVG_BPM), ("min_bpm", N.MR_MIN_BPM), ("max_bpm", N.MR_MAX_BPM),
                 ("avg_rmssdc", N.MR_AVG_RMSSDC), ("avg_sdnn", N.MR_AVG_SDNN)):
        if k in m["hrv_summary"]:
            rec[i] = m["hrv_summary"][k]
    h = m["hrr_stats"]
    if h is not None:
        p = _pos(s, h["peak_time"])
        assert h["peak_bpm"] == s.values[p] and p == int(np.argmax(s.values))
        assert h["recovery_check_time"] == h["peak_time"] + pd.Timedelta(seconds=60) and h["interval_sec"] == 60
        rec[N.MR_HRR_PEAK:N.MR_HRR_PEAK + 3] = (p, h["recovery_bpm"], h["hrr_value_bpm"])
    for k, i in (("peak_recovery_stats", N.MR_RECOVERY), ("peak_exertion_stats", N.MR_EXERTION)):
        d = m[k]
        if d is not None:
            a, b = _pos(s, d["start_time"]), _pos(s, d["end_time"])
            assert d["start_bpm"] == s.values[a] and d["end_bpm"] == s.values[b]
            rec[i:i + 4] = (a, b, d["slope_bpm_per_sec"], d["duration_sec"])
    df = m["windowed_hrv_df"]
    hrv = {c: (df[c].to_numpy(np.float64) if len(df) else np.zeros(0)) for c in HRV_COLS}
    return dict(record=rec, hrv=hrv,
                inc=None if m["major_inclines"] is None else _runs(s, m["major_inclines"], True),
                dec=None if m["major_declines"] is None else _runs(s, m["major_declines"], False))


def reference(c):
    """``beats.final_metrics`` on the case's beats -> (normal form or None when
    the reference makes no metrics, the dict itself).  When scipy rejects the
    distance, or the case brings its own curve, final_metrics' parts are called
    one by one (the runs left None in the first case)."""
    from bpm_analysis_amd.metrics import curve_series
    if c["bst"] != 0 or len(c["fin"]) < 2:
        return None, None
    peaks = c["fin"].astype(np.int64)
    with epoch(c["epoch_s"]):
        try:
            if c["custom"]:
                raise ValueError("distance: not yet known")
            m = B.final_metrics(peaks, c["sr"], c["params"])
        except ValueError as e:
            assert "distance" in str(e)
            m = {}
            if c["custom"]:
                m['smoothed_bpm'], m['bpm_times'] = s, _ = curve_series(c["bt"], c["bv"]), c["bt"]
            else:
                m['smoothed_bpm'], m['bpm_times'] = s, _ = B.bpm_series(peaks, c["sr"], c["params"])
            try:
                m['major_inclines'], m['major_declines'] = B.find_major_hr_inclines(s), B.find_major_hr_declines(s)
            except ValueError as e2:
                assert "distance" in str(e2)
                m['major_inclines'] = m['major_declines'] = None
            m['hrr_stats'] = B.calculate_hrr(s)
            m['peak_recovery_stats'] = B.find_peak_recovery_rate(s)
            m['peak_exertion_stats'] = B.find_peak_exertion_rate(s)
            m['windowed_hrv_df'] = h = B.windowed_hrv(peaks, c["sr"], c["params"])
            m['hrv_summary'] = dict(avg_bpm=s.mean(), min_bpm=s.min(), max_bpm=s.max())
            if not h.empty:
                m['hrv_summary'].update(avg_rmssdc=h['rmssdc'].mean(), avg_sdnn=h['sdnn'].mean())
    assert np.array_equal(m["smoothed_bpm"].values, c["bv"]) and np.array_equal(m["bpm_times"], c["bt"])
    return normal_form(m), m


def _same(a, b, bits, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = bool(np.array_equal(a, b, equal_nan=True))
    if bits:
        assert same, (what, a, b)
    else:
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        np.testing.assert_allclose(a, b, rtol=TB.RTOL, atol=0, equal_nan=True, err_msg=what)
    return same


POSITIONS = (N.MR_HRR_PEAK, N.MR_RECOVERY, N.MR_RECOVERY + 1, N.MR_EXERTION, N.MR_EXERTION + 1)


def assert_same(got, want, what="", bits=True, runs=True):
    """`got` (driver / device form) against a normal form: counts and positions
    equal, doubles bit-identical (``bits``) or within TB.RTOL.  Returns whether
    the doubles were bit-identical."""
    same = True
    for c in HRV_COLS:
        same &= _same(got["hrv"][c], want["hrv"][c], bits, (what, "hrv", c))
    gp, wp = got["record"][list(POSITIONS)], want["record"][list(POSITIONS)]
    assert np.array_equal(gp, wp, equal_nan=True), (what, "positions", gp, wp)
    same &= _same(got["record"], want["record"], bits, (what, "record"))
    for k in ("inc", "dec"):
        if not runs or want[k] is None:
            continue
        assert np.array_equal(got[k]["a"], want[k]["a"]) and np.array_equal(got[k]["b"], want[k]["b"]), (what, k)
        same &= _same(got[k]["slope"], want[k]["slope"], bits, (what, k, "slope"))
        same &= _same(got[k]["dur"], want[k]["dur"], bits, (what, k, "dur"))
    return same


def empty_form():
    z = np.zeros(0)
    zi = np.zeros(0, np.int32)
    return dict(record=np.full(N.METRICS_RECORD, np.nan), hrv={c: z for c in HRV_COLS},
                inc=dict(a=zi, b=zi, slope=z, dur=z), dec=dict(a=zi, b=zi, slope=z, dur=z))


def check(got, c, what="", bits=True):
    """One result against the reference, the status included -> bit-identical?"""
    want, _ = reference(c)
    if want is None:
        assert got["status"] == N.METRICS_NONE, what
        return assert_same(got, empty_form(), what, bits=True)
    st = got["status"]
    assert st >= 0 and st & ~(N.METRICS_TIE | N.METRICS_E_DISTANCE) == 0, (what, st)
    assert bool(st & N.METRICS_E_DISTANCE) == (want["inc"] is None), (what, st)
    if st & N.METRICS_E_DISTANCE:
        assert len(got["inc"]["a"]) == 0 and len(got["dec"]["a"]) == 0 and not st & N.METRICS_TIE, what
    # with a decisive tie numpy's argsort may visit in another order: the runs are then the host's business
    return assert_same(got, want, what, bits=bits, runs=not st & N.METRICS_TIE)


# ---- metrics_core_driver's files --------------------------------------------- #
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<iiiiq", len(c["fin"]), len(c["bt"]), c["sr"], c["bst"], c["epoch_s"] * 1000000))
            f.write(bytes(N.metric_params(c["params"])))
            f.write(c["fin"].tobytes() + c["bt"].tobytes() + c["bv"].tobytes())


def read_results(path, n_cases):
    buf = open(path, "rb").read()
    o, out = 0, []

    def take(dt, n):
        nonlocal o
        a = np.frombuffer(buf, dt, n, o)
        o += a.nbytes
        return a

    for _ in range(n_cases):
        st, nh, ni, nd = (int(v) for v in take(np.int32, 4))
        r = dict(status=st, record=take(np.float64, N.METRICS_RECORD))
        r["hrv"] = {c: take(np.float64, nh) for c in HRV_COLS}
        for k, n in (("inc", ni), ("dec", nd)):
            r[k] = dict(a=take(np.int32, n), b=take(np.int32, n), slope=take(np.float64, n), dur=take(np.float64, n))
        out.append(r)
    assert o == len(buf)
    return out


# ---- crafted inputs ----------------------------------------------------------- #
def with_params(w, step):
    return dict(PARAMS, hrv_window_size_beats=w, hrv_step_size_beats=step)


def crafted_cases():
    """[(name, case)] around every guard of the stage."""
    out = []
    rng = np.random.default_rng(11)

    def rr(n, lo=0.6, hi=1.0):
        return rng.uniform(lo, hi, n)

    for n in (0, 1, 2, 3):
        out.append((f"n{n}", case(beats_of(rr(max(n - 1, 0))) if n else np.zeros(0, np.int32))))
    for n in (39, 40, 41, 45, 46):                        # 0, 0, 1, 1, 2 HRV rows
        out.append((f"beats{n}", case(beats_of(rr(n - 1)))))
    for w in (7, 8, 9, 128, 129, 130):                    # every branch of the pairwise sum
        for step in (1, 5):
            out.append((f"w{w}_s{step}", case(beats_of(wander(w + 23, w)), params=with_params(w, step))))
    out.append(("win64", case(beats_of(rr(39 + 64)), params=with_params(40, 1))))      # 64 and 65 windows
    out.append(("win65", case(beats_of(rr(39 + 65)), params=with_params(40, 1))))
    out.append(("bad_status", case(beats_of(rr(60)), bst=-2)))
    # the 20 s guard of the steepest slopes: the curve lasts just under / just over 20 s
    for name, total in (("dur_under20", 19.99), ("dur_over20", 20.01)):
        r = rr(24)
        r[1:] *= total / r[1:].sum()
        out.append((name, case(beats_of(r))))
    # HRR: the curve ends just under / exactly 60 s past its maximum
    # (at 100 samples/s every beat time is a whole number of microseconds; the last beat is placed after the fact)
    for name, delta in (("hrr_under60", -1), ("hrr_exact60", 0)):
        fin = beats_of(np.concatenate([np.linspace(1.0, 0.45, 30), np.linspace(0.5, 1.0, 60)]), sr=100, t0=1.0)
        am = int(np.argmax(case(fin, sr=100)["bv"]))
        end = int(fin[am + 1]) + 60 * 100 + delta
        c = case(np.append(fin[fin < end - 50], end), sr=100)
        assert int(np.argmax(c["bv"])) == am and c["bt"][am] == fin[am + 1] / 100
        out.append((name, c))
    out.append(("max_is_last", case(beats_of(np.linspace(1.0, 0.4, 60)))))
    v = 70 + 10 * np.sin(np.arange(100) / 7.0)             # a curve of its own: two equal maxima, the first idxmax counts
    v[[20, 33]] = 131.25
    out.append(("two_equal_maxima", case((np.arange(101) * SR + 9).astype(np.int32),
                                         curve=(np.arange(1, 101, dtype=np.float64), v))))
    out.append(("constant_rr", case(beats_of(np.full(120, 0.5), sr=100, t0=1.0), sr=100)))   # exactly 120 BPM
    out.append(("slow_step_over_5s", case(beats_of(rng.uniform(5.2, 6.5, 50)))))
    for off in (3600, -18000):
        r = np.concatenate([np.linspace(1.0, 0.45, 40), np.linspace(0.45, 1.0, 150)]) * rng.uniform(0.97, 1.03, 190)
        out.append((f"epoch{off}", case(beats_of(r), epoch_s=off)))
    for seed in range(6):                                 # inclines and declines, several of each
        out.append((f"wander{seed}", case(beats_of(wander(500 + 40 * seed, seed, period=50.0 + 9 * seed)))))
    out.append(("long605", case(beats_of(wander(604, 9, lo=500.0, hi=640.0, period=20.0, noise=0.01)))))
    return out


def tie_cases(n=200, seed=5):
    """Small curves on a grid of 0.5 BPM, one point per second (distance 5):
    equal heights within the distance are common."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(20, 61))
        lvl = 60 + 30 * np.sin(np.arange(m) / rng.uniform(3, 9) + rng.uniform(0, 6))
        v = np.round((lvl + rng.integers(0, 5, m) * rng.choice([0.5, 3.0])) * 2) / 2
        fin = (np.arange(m + 1) * SR + SR // 2).astype(np.int32)
        out.append((f"tie{k}", case(fin, curve=(np.arange(1, m + 1, dtype=np.float64), v))))
    return out
