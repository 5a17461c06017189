"""Recordings for the native-envelope format tests (tests/test_oracle.py pins
the oracle on them against scipy, tests/test_gpu_native_formats.py the GPU
against the oracle): every sample format scipy.io.wavfile gives, one to three
channels, with edges that make scipy's odd extension matter.

sosfiltfilt pads with odd_ext, which evaluates 2 * end - x[k] in the array's
own dtype: mono u8 / int16 / int32 wrap around, float32 rounds, and a
multi-channel integer recording (np.mean -> float64) does neither.  The first
and last 17 frames are therefore random over the format's full range, frame 0
near the top and the last frame near the bottom, so that 2 * end - x[k]
leaves the range at both ends for nearly every k; float32 edges spread their
magnitudes over 2^-12 ... 1, so that the rounding of 2 * end - x[k] differs
from double's by up to half an ulp of 2."""
import numpy as np

from oracle import oracle as O

NP_DT = {"u8": np.uint8, "i16": np.int16, "i32": np.int32, "f32": np.float32, "f64": np.float64}
EDGE = 17                          # filtfilt's pad reads x[1 .. 15] and x[-16 .. -2]; the ends scale them
F64_SCALE = np.sqrt(2.0) / 32768   # an irrational scale: no float64 sample is a short binary fraction


def rate(ds):
    """fs = 320 ds: downsample_factor = ds is then exactly the decimation
    (sr 320, envelope window 32) for every ds >= 31."""
    return 320 * ds


def params(ds):
    from tests import goldens as G
    return dict(G.BASE_PARAMS, downsample_factor=ds)


def _edges(rng, dtype, ch):
    """(head, tail): EDGE frames each, [EDGE, ch]."""
    if dtype in ("u8", "i16", "i32"):
        ii = np.iinfo(NP_DT[dtype])
        span = int(ii.max) - int(ii.min)
        head = rng.integers(ii.min, int(ii.max) + 1, (EDGE, ch))
        tail = rng.integers(ii.min, int(ii.max) + 1, (EDGE, ch))
        head[0] = int(ii.max) - rng.integers(0, span // 64 + 1, ch)
        tail[-1] = int(ii.min) + rng.integers(0, span // 64 + 1, ch)
        return head, tail
    out = []
    for _ in range(2):
        mag = 2.0 ** (-12.0 * rng.random((EDGE, ch))) * (0.5 + 0.5 * rng.random((EDGE, ch)))
        out.append(np.where(rng.random((EDGE, ch)) < 0.5, -mag, mag))
    head, tail = out
    head[0] = 0.97 + 0.03 * rng.random(ch)
    tail[-1] = -(0.97 + 0.03 * rng.random(ch))
    if dtype == "f64":
        head, tail = head * np.sqrt(2.0), tail * np.sqrt(2.0)
    return head, tail


def recording(dtype, ch, n, fs, seed, edges=True):
    """[n] or [n, ch] samples of `dtype`: the oracle's synthetic heart sounds
    at half scale plus uniform noise in +-8000 (int16 units), mapped to the
    format; channels 1 and 2 are the reversed and a rolled copy, so the mean
    is no copy of a channel."""
    rng = np.random.default_rng(seed)
    b = O.synth(seed, n, fs, 1).astype(np.int64) // 2 + rng.integers(-8000, 8001, n)
    x = np.stack([b, b[::-1], np.roll(b, n // 3)][:ch], axis=1)
    if dtype == "u8":
        x = (x >> 8) + 128
    elif dtype == "i32":
        x = x * 65536 + rng.integers(0, 65536, x.shape)
    elif dtype == "f32":
        x = x / 32768.0
    elif dtype == "f64":
        x = x * F64_SCALE
    x = x.astype(NP_DT[dtype])
    if edges:
        head, tail = _edges(rng, dtype, ch)
        x[:EDGE], x[-EDGE:] = head.astype(NP_DT[dtype]), tail.astype(NP_DT[dtype])
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


def cast_y(x, d):
    """The oracle's decimated signal for the same samples cast to float64
    first: no wrap, no float32 rounding, a float64 channel mean."""
    return O.preprocess_native(x.astype(np.float64), d, return_y=True)[1]


def discrimination(y, y_cast):
    """D = max |y - y_cast| / max |y|."""
    return float(np.max(np.abs(y - y_cast)) / np.max(np.abs(y)))
