"""tests/ref_cases.py without a GPU: the case table is the cover it claims,
every length set sits on the switches of ref_env_plan (read through
tests/plan_driver.hip, as tests/test_plan.py does), the oracle equals scipy's
filtfilt and pandas' centred rolling mean bit for bit on the recordings the
GPU is then compared on, and those recordings meet the conditions that make a
wrong kernel fail: with y_cast the oracle's y for the samples cast to float64
first and D = max |y - y_cast| / max |y|,
* mono u8 / int16 / int32: D >= 1e-3 for every recording (the odd
  extension's wrap-around decides the result);
* multi-channel integers: y == y_cast exactly, while channel 0 alone has
  D >= 1e-3 (a kernel that wraps there is far off);
* float32: D >= 3e-9 (a kernel that extends or averages in double differs);
* float64: equal.
The GPU comparison itself is exact."""
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from tests import ref_cases as RC
from tests.test_plan import OPT_REF_NOSPLIT, OPT_REF_SERIAL_MEAN, _has, driver  # noqa: F401 (driver: a fixture)

D_INT, D_F32 = 1e-3, 3e-9


def library(x, w):
    """The reference's calls on one recording: np.mean over the channels,
    x[::ds], butter, filtfilt, |y|, rolling(w, min_periods=1, center=True).mean()."""
    import pandas as pd
    from scipy.signal import butter, filtfilt
    _, ds, sr = RC.RATES[w]
    if x.ndim > 1:
        x = np.mean(x, axis=1)
    nyq = 0.5 * sr
    b, a = butter(2, [20 / nyq, 150 / nyq], btype="band")
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        y = filtfilt(b, a, x[::ds])
        env = pd.Series(np.abs(y)).rolling(window=sr // 10, min_periods=1, center=True).mean().values
    return env, y


def _oracle_is_library(x, w, what):
    env, y = O.preprocess_ref(x, RC.derived(w), return_y=True)
    want_env, want_y = library(x, w)
    assert np.array_equal(y, want_y, equal_nan=True), ("y", what)
    assert np.array_equal(env, want_env, equal_nan=True), ("env", what)
    return env, y


def test_rates():
    for w, (fs, ds, sr) in RC.RATES.items():
        d = RC.derived(w)
        assert (d.ds, d.sr, d.env_w) == (ds, sr, w)
    assert [w for w in RC.RATES if w > RC.PF] == [44, 220] and 220 > 2 * RC.PF * 3


def test_case_table_is_a_cover():
    have = {(c.rate, c.dtype, c.ch > 1, c.set) for c in RC.REF_CASES}
    for rate in (30, 32):
        for dt in RC.DTYPES:
            for multi in (False, True):
                assert (rate, dt, multi, "kahan") in have
    for rate in RC.RATES:
        for dt, multi in (("i16", False), ("f32", True), ("f64", False)):
            for s in ("small", "split", "kahan"):
                assert (rate, dt, multi, s) in have
    assert any(c.set == "kahan4096" for c in RC.REF_CASES)
    three = {(c.rate, c.dtype) for c in RC.REF_CASES if c.ch == 3}
    assert any({(r, "i16"), (r, "f32"), (r, "f64")} <= three for r in RC.RATES)
    for s in ("kahan", "small"):
        assert {RC.CHAIN_W[c.rate] for c in RC.REF_CASES if c.set == s} == {30, 31, 32, 0}
    assert all(c.off == 0 or c.off % 2 == 1 for c in RC.REF_CASES)
    assert {c.off == 0 for c in RC.REF_CASES} == {False, True}
    assert all(c.set in RC.SETS and c.rate in RC.RATES and c.dtype in RC.DTYPES for c in RC.REF_CASES)


def test_length_sets():
    for w in RC.RATES:
        off = (w - 1) // 2
        want = {"small": {16, 17, w - 1, w, w + 1, 2 * w + 1, 63, 64, 65, 127, 129, 900},
                "split": {16, w, 994, 995, 1023, 1025, 3042, 3043, 4095}}
        ke = RC.kend(RC.MAXND)
        assert ke == [3520, 5312, 6208, 7141]
        want["kahan"] = {4096, 16, w + 1, RC.MAXND} | {ke[k] + o for k in range(3) for o in (-1, 0, 1, off + 1)}
        for s in RC.SETS:
            nds = RC.set_nds(s, w)
            assert len(nds) == RC.F == 70 and nds.count(15) == 1
            if s in want:
                assert set(nds) - {15} == want[s], (w, s)
            w0, w1 = nds[:RC.WAVE], nds[RC.WAVE:]
            assert set(w0) == set(nds) and len(w1) == 6 and len(set(w1)) == 6, (w, s)   # both waves ragged
            # wave 0: a lane ends in the first block beside the longest, so the wave never
            # meets `i0 + PF + off <= ndmin`: the predicated branches only
            assert min(n for n in w0 if n > 15) == 16 and 16 < RC.PF + off
            if s != "small":
                # wave 1: blocks i0 in [w - off, ndmin - PF - off] are steady state (several of
                # them, the prefetch's `i0 + 2 PF + off <= ndmin` among them), then ragged ends
                first = -(-(w - off) // RC.PF) * RC.PF
                assert min(w1) >= 994 and first + 4 * RC.PF + off <= min(w1) < max(w1), (w, s)
            if s.startswith("kahan"):
                # and for wave 1 so are the first blocks of k_ref_kahan's chunk from ib = kend[0]
                assert RC.kend(max(nds))[0] + 4 * RC.PF + off <= min(w1), (w, s)
            if s == "small":
                assert max(nds) < 995 and min(w1) == 16
            elif s == "split":
                assert 995 <= max(nds) < RC.KAHAN_MIN
                assert {n + 30 for n in nds} >= {RC.FWD_ROWS, RC.FWD_ROWS + 1, 3 * RC.FWD_ROWS, 3 * RC.FWD_ROWS + 1}
            elif s == "kahan":
                assert max(nds) == RC.MAXND and RC.MAXND + 30 == 7 * RC.FWD_ROWS + 3
            else:
                assert max(nds) == RC.KAHAN_MIN
        # 16 <= nd < w: the window outlasts the recording
        assert 16 <= w - 1 and RC.set_nds("small", w).count(w - 1) >= 1


def test_sets_sit_on_the_plan_switches(driver):  # noqa: F811
    keys = [(w, s) for w in RC.RATES for s in RC.SETS]
    plans = dict(zip(keys, driver(*[f"ref:{max(RC.set_nds(s, w))}:{w}:0" for w, s in keys])))
    for (w, s), p in plans.items():
        maxnd = max(RC.set_nds(s, w))
        rows = maxnd + 30
        nfc = 1
        while min(rows, RC.FWD_ROWS * (2 ** nfc - 1)) < rows:
            nfc += 1
        fwd = ",".join(str(min(rows, RC.FWD_ROWS * (2 ** k - 1))) for k in range(nfc + 1))
        _has(p, chain=1, rows=rows, nfc=nfc, fwd=fwd)
        if s == "small":
            _has(p, nfc=1, wants_split=0, nkc=0, kend="", fwd=f"0,{rows}")
        elif s == "split":
            _has(p, nfc=3, wants_split=1, nkc=0, kend="", fwd="0,1024,3072,4125")
        elif s == "kahan":
            _has(p, nfc=4, wants_split=1, nkc=4, kend="3520,5312,6208,7141", fwd="0,1024,3072,7168,7171")
        else:
            _has(p, nfc=3, wants_split=1, nkc=4, kend="2048,3072,3584,4096", fwd="0,1024,3072,4126")
        if s.startswith("kahan"):
            assert p["kend"] == ",".join(map(str, RC.kend(maxnd)))
    below, nosplit, serial = driver("ref:4095:31:0", f"ref:{RC.MAXND}:44:{OPT_REF_NOSPLIT}",
                                    f"ref:{RC.MAXND}:220:{OPT_REF_SERIAL_MEAN}")
    _has(below, nkc=0, wants_split=1)
    _has(nosplit, wants_split=0, nkc=0, chain=1)
    _has(serial, chain=0, nkc=0, wants_split=1)


def test_recording_lengths_and_edges():
    for dt, ch in (("u8", 1), ("i32", 2), ("f32", 3), ("f64", 1)):
        for nd in (15, 16, 17, 33, 900):
            for tail in ("min", "max"):
                x = RC.recording(dt, ch, nd, 20, 77, tail)
                assert x.dtype == RC.NP_DT[dt] and x.shape == (((nd - 1) * 20 + 1 if tail == "min" else nd * 20),) + \
                    ((ch,) if ch > 1 else ())
                assert RC.nd_of(x, 20) == nd
                top, bottom = x[0].astype(np.float64), x[(nd - 1) * 20].astype(np.float64)
                if dt in ("u8", "i32"):
                    ii = np.iinfo(RC.NP_DT[dt])
                    span = float(ii.max) - float(ii.min)
                    assert np.all(top >= ii.max - span / 64) and np.all(bottom <= ii.min + span / 64)
                else:
                    assert np.all(top >= 0.97) and np.all(bottom <= -0.97)


_small = {}


def _small_set(rate, dtype, ch):
    """One `small` set per (rate, format, channels) of the table, with the oracle's answers."""
    key = (rate, dtype, ch)
    if key not in _small:
        fs, ds, _ = RC.RATES[rate]
        recs = [RC.recording(dtype, ch, nd, ds, 31000 + 100 * len(_small) + i, "max" if i % 2 else "min", fs)
                for i, nd in enumerate(RC.set_nds("small", rate)) if nd > 15]
        _small[key] = recs
    return _small[key]


TRIPLES = sorted({(c.rate, c.dtype, c.ch) for c in RC.REF_CASES})


@pytest.mark.parametrize("rate,dtype,ch", TRIPLES, ids=[f"w{r}-{d}x{c}" for r, d, c in TRIPLES])
def test_oracle_matches_libraries_and_inputs_discriminate(rate, dtype, ch):
    d = RC.derived(rate)
    integer = dtype in ("u8", "i16", "i32")
    worst = None
    for k, x in enumerate(_small_set(rate, dtype, ch)):
        _, y = _oracle_is_library(x, rate, (rate, dtype, ch, k))
        dist = RC.discrimination(y, RC.cast_y(x, d))
        worst = dist if worst is None else min(worst, dist)
        if integer and ch == 1:
            assert dist >= D_INT, (k, dist)
        elif integer:
            x0 = np.ascontiguousarray(x[:, 0])
            d0 = RC.discrimination(O.preprocess_ref(x0, d, return_y=True)[1], RC.cast_y(x0, d))
            assert dist == 0.0 and d0 >= D_INT, (k, dist, d0)
        elif dtype == "f32":
            assert dist >= D_F32, (k, dist)
        else:
            assert dist == 0.0, k
    print(f"w{rate} {dtype}x{ch}: smallest D {worst:.3e}")


@pytest.mark.parametrize("w", list(RC.RATES))
def test_special_recordings(w):
    fs, ds, _ = RC.RATES[w]
    # few ulps of the smallest subnormal: runs of equal |y| shorter and longer than the window
    x = RC.few_ulp_for(w)
    _, y = _oracle_is_library(x, w, ("few_ulp", w))
    n2, nw, npart, longest = RC.few_ulp_stats(y, w)
    print(f"few_ulp w{w} seed {RC.FEW_ULP[w]}: runs>=2 {n2} runs>=w {nw} runs in [2,w) {npart} longest {longest}")
    assert n2 >= 100 and nw >= 1 and npart >= 1 and np.max(np.abs(y)) > 0
    assert RC.few_ulp_condition(y, w) and (n2, nw, longest) == RC.FEW_ULP_RUNS[w]
    assert np.max(np.abs(y)) < 2.0 ** -1060
    # float64 subnormals
    x = RC.subnormal_f64(3, fs)
    _, y = _oracle_is_library(x, w, ("subnormal_f64", w))
    ay = np.abs(y[y != 0])
    assert ay.size > y.size // 2 and np.all(ay < RC.DBL_MIN)
    # float32 subnormals, mono and stereo
    for ch in (1, 2):
        x = RC.subnormal_f32(4, fs, ch)
        ax = np.abs(x[x != 0])
        assert x.dtype == np.float32 and ax.size > x.size // 2 and np.all(ax < RC.FLT_MIN)
        _, y = _oracle_is_library(x, w, ("subnormal_f32", w, ch))
        assert 0 < np.max(np.abs(y)) < RC.FLT_MIN          # a flushed sample or channel mean would give zeros
    # one NaN or +Inf: y and env NaN at every index
    for dtype in ("f32", "f64"):
        for kind, pos in RC.NONFINITE:
            for nd in (16, 995):
                x = RC.nonfinite(kind, pos, dtype, nd, ds, 5, fs)
                assert np.sum(~np.isfinite(x)) == 1 and not np.isfinite(x[::ds]).all()
                env, y = _oracle_is_library(x, w, (kind, pos, dtype, nd))
                assert y.size == nd and np.isnan(y).all() and np.isnan(env).all(), (kind, pos, dtype, nd)
