"""Recordings and the case table of the reference-envelope sweep
(tests/test_ref_cases.py keeps the table a cover of the reference kernels'
branches and pins the oracle on every input against scipy and pandas;
tests/test_gpu_ref_formats.py compares the GPU with the oracle, bit for bit).

Reference mode is x[::ds] -> filtfilt(b, a) -> |y| -> centred rolling mean of
sr // 10 samples.  filtfilt pads the *decimated* signal with odd_ext, which
evaluates 2 * end - x[k] in the array's own dtype (mono u8 / int16 / int32
wrap around, float32 rounds, a multi-channel integer recording has become
float64 by np.mean and does neither), so the frames that decide a result are
k ds and (nd - 1 - k) ds, not a recording's first and last frames: recording()
puts tests/native_cases.py's edge values there.

The envelope window is sr // 10 and the 150 Hz band edge forces sr > 300, so
no window below 30 can be reached through the library's own filter design
(w == 1 least of all); nor can an integer format meet a numerator that is not
k (1, 0, -2, 0, 1) (ZB = false in k_envelope_ref.hip).  Both stay untested.

No GPU and no torch in this module."""
import collections

import numpy as np

from oracle import oracle as O
from tests import goldens as G
from tests.native_cases import EDGE, F64_SCALE, NP_DT, _edges

DTYPES = ("u8", "i16", "i32", "f32", "f64")
PF = 32                            # k_envelope_ref.hip: the rolling mean's prefetch block
FWD_ROWS = 1024                    # bpmx_plan.h REF_FWD_ROWS: forward chunk k ends at row 1024 (2^(k+1) - 1)
KAHAN_MIN = 4096                   # ref_env_plan: the Kahan pass runs in row chunks from this maxnd on
F = 70                             # recordings per set: one full wave and six lanes of a second
WAVE = 64

# envelope window -> (fs, downsample_factor, sr)
RATES = {30: (44100, 146, 302), 31: (44100, 140, 315), 32: (320 * 146, 146, 320), 44: (44100, 100, 441),
         220: (44100, 20, 2205)}
# the kahan_chain<W> instantiation a window runs (k_ref_kahan's switch)
CHAIN_W = {30: 30, 31: 31, 32: 32, 44: 0, 220: 0}


def params(w):
    return dict(G.BASE_PARAMS, downsample_factor=RATES[w][1])


def derived(w):
    fs, ds, sr = RATES[w]
    d = O.derive(fs, params(w))
    assert (d.ds, d.sr, d.env_w) == (ds, sr, w)
    return d


def recording(dtype, ch, nd, ds, seed, tail="min", fs=44100):
    """[n] or [n, ch] samples of `dtype` that decimate to nd samples: n =
    (nd - 1) ds + 1 (tail "min": the last pick is the last frame) or nd ds
    ("max").  tests/native_cases.py's recipe (the oracle's synthetic heart
    sounds at half scale plus uniform noise in +-8000, mapped to the format;
    channels 1 and 2 the reversed and a rolled copy), with its edge values on
    the decimated grid: frames k ds and (nd - 1 - k) ds for k < min(17, nd)
    are random over the format's full range (float32: magnitudes spread over
    2^-12 ... 1), frame 0 near the top, frame (nd - 1) ds near the bottom."""
    n = (nd - 1) * ds + 1 if tail == "min" else nd * ds
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
    head, end = _edges(rng, dtype, ch)
    m = min(EDGE, nd)
    x[np.arange(m) * ds] = head[:m].astype(NP_DT[dtype])
    x[(nd - m + np.arange(m)) * ds] = end[EDGE - m:].astype(NP_DT[dtype])
    x[0] = head[0].astype(NP_DT[dtype])
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


def nd_of(x, ds):
    return -(-x.shape[0] // ds)


# ---- length sets ----
MAXND = 7141                       # rows = 7171: three rows into forward chunk 3 (rows 7168 ...)
SETS = ("small", "split", "kahan", "kahan4096")


def kend(maxnd):
    """ref_env_plan's Kahan chunk ends (tests/test_ref_cases.py holds them against the plan itself)."""
    return [(maxnd - (maxnd >> k)) & ~63 for k in (1, 2, 3)] + [maxnd]


def set_lengths(name, w):
    """(the distinct decimated lengths of a set, the six of them that wave 1 repeats)."""
    off = (w - 1) // 2
    if name == "small":                 # maxnd < 995: one forward chunk, no split
        return [16, 17, w - 1, w, w + 1, 2 * w + 1, 63, 64, 65, 127, 129, 900], [129, 16, 900, w - 1, 2 * w + 1, 64]
    if name == "split":                 # 995 <= maxnd < 4096: rows 1024, 1025, 3072, 3073 are forward chunk ends
        return [16, w, 994, 995, 1023, 1025, 3042, 3043, 4095], [3043, 994, 1025, 3042, 995, 1023]
    if name == "kahan":                 # maxnd >= 4096: the Kahan pass in row chunks
        ke = kend(MAXND)
        nds = [n for k in range(3) for n in (ke[k] - 1, ke[k], ke[k] + 1, ke[k] + off + 1)]
        # wave 1 ends in Kahan chunks 2 and 3: chunk 1 (k_ref_kahan from ib = kend[0]) is steady state for it
        return nds + [KAHAN_MIN, 16, w + 1, MAXND], [ke[2] + 1, ke[1] - 1, ke[1] + 1, ke[2], ke[1] + off + 1, ke[2] - 1]
    ke = kend(KAHAN_MIN)                # the switch itself
    return ([ke[0] - 1, ke[0], ke[0] + off + 1, ke[1] - 1, ke[1] + 1, ke[2], ke[2] + 1, KAHAN_MIN - 1, KAHAN_MIN, 16,
             w + 1], [ke[1] + 1, ke[1] - 1, ke[2], ke[2] + 1, KAHAN_MIN - 1, KAHAN_MIN])


SHORT = 1000                       # wave 0 is filled with copies of the set's lengths below this


def set_nds(name, w):
    """The F decimated lengths of a set in batch order.  Wave 0: every distinct
    length, spread evenly over the lanes, one recording of 15 (too short, the
    library's F_TOO_SHORT) at lane 2 and copies of the short lengths elsewhere,
    so a lane ends in the first block beside the longest and the wave only
    ever takes the predicated branches.  Wave 1 (six lanes): second copies of
    six lengths, in the longer sets all of them long, so that its shortest
    recording is far inside the steady state and the others end ragged."""
    base, wave1 = set_lengths(name, w)
    base = list(dict.fromkeys(base))
    assert len(wave1) == F - WAVE and set(wave1) <= set(base)
    short = [n for n in base if n < SHORT]
    out = [None] * WAVE
    for j, n in enumerate(base):
        out[WAVE - 1 - (j * WAVE) // len(base)] = n
    assert out[2] is None
    out[2] = 15
    k = 0
    for i in range(WAVE):
        if out[i] is None:
            out[i] = short[k % len(short)]
            k += 1
    return out + wave1


Case = collections.namedtuple("Case", "name rate dtype ch set off")


def _case(rate, dtype, ch, set_, off=None):
    name = f"w{rate}-{dtype}x{ch}-{set_}"
    if off is None:                     # 0 or an odd element offset, fixed by the name
        off = (0, 1, 3, 5, 7, 0, 9, 11)[sum(name.encode()) % 8]
    return Case(name, rate, dtype, ch, set_, off)


def _table():
    t = []
    for rate in (30, 32):               # every format, mono and stereo, through the chunked Kahan pass
        for dt in DTYPES:
            for ch in (1, 2):
                t.append(_case(rate, dt, ch, "kahan"))
    for rate in RATES:                  # every window through every set
        for dt, ch in (("i16", 1), ("f32", 2), ("f64", 1)):
            for s in ("small", "split", "kahan"):
                t.append(_case(rate, dt, ch, s))
        t.append(_case(rate, "i16", 1, "kahan4096"))
    for dt in ("i16", "f32", "f64"):    # three channels
        t.append(_case(31, dt, 3, "split"))
    return list(dict.fromkeys(t))


REF_CASES = _table()
CASES = {c.name: c for c in REF_CASES}
assert len(CASES) == len(REF_CASES)
# with this base every float32 recording has D >= 3e-9 (mono ones of 16 samples come closest, 4e-9)
SEED0 = 9008


def case_recordings(c):
    """The case's F recordings in batch order (tail "min" and "max" alternate)."""
    fs, ds, _ = RATES[c.rate]
    base = SEED0 + 100 * REF_CASES.index(c)
    return [recording(c.dtype, c.ch, nd, ds, base + i, "max" if i % 2 else "min", fs)
            for i, nd in enumerate(set_nds(c.set, c.rate))]


def cast_y(x, d):
    """The oracle's y for the same samples cast to float64 first: no wrap, no
    float32 rounding, a float64 channel mean."""
    return O.preprocess_ref(x.astype(np.float64), d, return_y=True)[1]


def discrimination(y, y_cast):
    """D = max |y - y_cast| / max |y|."""
    return float(np.max(np.abs(y - y_cast)) / np.max(np.abs(y)))


# ---- special recordings ----
DBL_MIN = float(np.finfo(np.float64).tiny)
FLT_MIN = float(np.finfo(np.float32).tiny)
# few_ulp's (seed, second exponent) per window and what the oracle's |y| then holds over 8 s:
# (runs >= 2, runs >= w, longest run); tests/test_ref_cases.py asserts these figures.  At
# sr 2205 b0 is 0.027 and the recipe's samples are at most 3 ulps, so b0 x rounds to zero
# and y is all zero with 2^-85; 2^-83 is the smallest scale with a nonzero y.
FEW_ULP = {30: (5, -85), 31: (5, -85), 32: (5, -85), 44: (5, -85), 220: (5, -83)}
FEW_ULP_RUNS = {30: (318, 5, 98), 31: (170, 8, 89), 32: (185, 3, 84), 44: (176, 31, 181), 220: (317, 5, 832)}


def runs(v):
    """Lengths of the maximal runs of equal consecutive values."""
    v = np.asarray(v)
    cut = np.flatnonzero(v[1:] != v[:-1]) + 1
    return np.diff(np.concatenate([[0], cut, [v.size]]))


def few_ulp(seed, ds, fs, secs=8, exp=-85):
    """float64 mono, a few ulps of the smallest subnormal: (synth 2^-1000)
    2^exp (in two steps: 2.0 ** -1085 is 0), ending on its last pick.
    Condition (few_ulp_condition): |y| has at least 100 runs of two or more
    equal consecutive values, one of them at least w long and one of a length
    in [2, w), and is not all zero: k_ref_env_mean's count of the run ending
    at the last added value then stops both at nobs and before it."""
    x = (O.synth(seed, secs * fs, fs, 1).astype(np.float64) * 2.0 ** -1000) * 2.0 ** exp
    return np.ascontiguousarray(x[:(secs * fs - 1) // ds * ds + 1])


def few_ulp_for(w, secs=8):
    fs, ds, _ = RATES[w]
    return few_ulp(FEW_ULP[w][0], ds, fs, secs, FEW_ULP[w][1])


def few_ulp_stats(y, w):
    r = runs(np.abs(y))
    return int(np.sum(r >= 2)), int(np.sum(r >= w)), int(np.sum((r >= 2) & (r < w))), int(r.max())


def few_ulp_condition(y, w):
    n2, nw, npart, _ = few_ulp_stats(y, w)
    return n2 >= 100 and nw >= 1 and npart >= 1 and float(np.max(np.abs(y))) > 0


def subnormal_f64(seed, fs, secs=8):
    """float64 mono, synth 2^-1040.  Condition: every nonzero |y| is below DBL_MIN."""
    return O.synth(seed, secs * fs, fs, 1).astype(np.float64) * 2.0 ** -1040


def subnormal_f32(seed, fs, ch=1, secs=8):
    """float32, (synth 2^-145).astype(float32), channel 1 the reversed copy.
    Condition: every nonzero sample is a float32 subnormal (the stereo mean is
    then formed in float32 subnormals)."""
    b = O.synth(seed, secs * fs, fs, 1).astype(np.float64) * 2.0 ** -145
    x = np.stack([b, b[::-1]][:ch], axis=1).astype(np.float32)
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


NONFINITE = [(kind, pos) for pos in ("middle", "first", "pad", "last") for kind in ("nan", "inf")]


def nonfinite(kind, pos, dtype, nd, ds, seed, fs=44100):
    """A float32 or float64 mono recording with one NaN or +Inf on the
    decimated grid: in the middle, at frame 0, at frame 3 ds (which the odd
    extension also puts into the head pad) or at the last pick.  Condition,
    checked against scipy and pandas: y and env are NaN at every index."""
    x = recording(dtype, 1, nd, ds, seed, "max", fs)
    at = {"middle": nd // 2, "first": 0, "pad": 3, "last": nd - 1}[pos]
    x[at * ds] = np.nan if kind == "nan" else np.inf
    return x
