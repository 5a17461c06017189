"""Inputs and the expected envelope for the rectified mode's tests.

The expected envelope is the labeler's recipe itself (heartbeat_labeler.py
:53-67), made with the libraries the reference calls: channel mean for more
than one channel, ``np.abs`` in that dtype, the centred pandas rolling mean."""
import os
import re
import struct

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_constants():
    """RECT_T, RECT_CHUNK and RECT_LDS_N as csrc/bpmx_kernels.h states them
    (tests/test_rect_plan.py checks them against the compiled plan)."""
    with open(os.path.join(REPO, "bpm_analysis_amd", "csrc", "bpmx_kernels.h")) as f:
        text = f.read()
    out = {}
    for name in ("RECT_T", "RECT_CHUNK", "RECT_LDS_N"):
        out[name] = int(re.search(r"constexpr \w+ %s = (\d+);" % name, text).group(1))
    return out

DTYPES = {"u8": (np.uint8, 0), "i16": (np.int16, 1), "i32": (np.int32, 2), "f32": (np.float32, 3),
          "f64": (np.float64, 4)}
INT_NAMES = ("u8", "i16", "i32")
FLOAT_NAMES = ("f32", "f64")


def recipe(pcm, w):
    """pcm: [n] (mono, as wavfile.read gives it) or [n, C]."""
    import pandas as pd
    with np.errstate(invalid="ignore"):                 # inf + -inf in a generated frame
        x = pcm if pcm.ndim == 1 else np.mean(pcm, axis=1)
    a = np.abs(x)
    if len(a) == 0:
        return np.zeros(0)
    return pd.Series(a).rolling(window=int(w), min_periods=1, center=True).mean().to_numpy()


def same_bits(got, want):
    """uint64 patterns where the result is not NaN, NaN positions otherwise."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~wn], want.view(np.uint64)[~wn]))


def shape(x, ch):
    """[n, C] -> what wavfile.read returns: [n] for one channel."""
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


def make_int(rng, name, n, ch, kind="random"):
    dt = DTYPES[name][0]
    info = np.iinfo(dt)
    if kind == "allmin":
        return shape(np.full((n, ch), info.min, dtype=dt), ch)
    if kind == "zeros":
        return shape(np.zeros((n, ch), dtype=dt), ch)
    x = rng.integers(info.min, int(info.max) + 1, size=(n, ch), dtype=np.int64).astype(dt)
    if n == 0:
        return shape(x, ch)
    # minimum-value samples (np.abs leaves them negative) and runs of equal values
    x[rng.random((n, ch)) < 0.05] = info.min
    for _ in range(max(1, n // 40)):
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(1, 40)))
        x[a:b] = x[a]
    if n > 8:
        a = int(rng.integers(0, n - 4))
        x[a:a + int(rng.integers(2, 6))] = info.min
    return shape(x, ch)


def make_float(rng, name, n, ch):
    dt = DTYPES[name][0]
    x = (rng.standard_normal((n, ch)) * 0.3).astype(dt)
    if n == 0:
        return shape(x, ch)
    r = rng.random((n, ch))
    tiny = np.finfo(dt).tiny
    x[r < 0.03] = np.nan
    x[(r >= 0.03) & (r < 0.05)] = np.inf
    x[(r >= 0.05) & (r < 0.07)] = -np.inf
    x[(r >= 0.07) & (r < 0.10)] = -0.0
    x[(r >= 0.10) & (r < 0.13)] = dt(tiny / 8)          # denormal
    x[(r >= 0.13) & (r < 0.15)] = dt(-tiny / 4)
    for _ in range(max(1, n // 50)):
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(1, 40)))
        x[a:b] = x[a]
    return shape(x, ch)


def make(rng, name, n, ch, kind="random"):
    return make_int(rng, name, n, ch, kind) if name in INT_NAMES else make_float(rng, name, n, ch)


def write_cases(path, cases):
    """cases: (pcm array, window); the format of tests/rect_core_driver.cpp."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for pcm, w in cases:
            code = next(c for t, c in DTYPES.values() if t == pcm.dtype.type)
            ch = 1 if pcm.ndim == 1 else pcm.shape[1]
            f.write(struct.pack("<iiiiq", code, ch, int(w), 0, pcm.shape[0]))
            f.write(np.ascontiguousarray(pcm).tobytes())


def read_results(path, cases):
    """-> per case (general, exact or None)"""
    out = []
    with open(path, "rb") as f:
        for pcm, _ in cases:
            n = pcm.shape[0]
            has, _pad = struct.unpack("<ii", f.read(8))
            gen = np.frombuffer(f.read(8 * n), dtype=np.float64)
            ex = np.frombuffer(f.read(8 * n), dtype=np.float64) if has else None
            out.append((gen, ex))
        assert f.read() == b""
    return out
