"""Shared by test_beats_core.py (CPU) and test_gpu_beats.py: crafted per-peak
tables, the comparison against ``_host.beats_packed`` and against the
reference's beat goldens, and the binary exchange with beats_core_driver."""
from __future__ import annotations

import ctypes
import functools
import struct

import numpy as np

from bpm_analysis_amd import DEFAULT_PARAMS
from bpm_analysis_amd import _host as H
from bpm_analysis_amd import beats as B
from tests import test_beats as TB

SR = 302                               # 44100 // 146, the default decimated rate
PARAMS = dict(DEFAULT_PARAMS, save_filtered_wav=False)
SMALL_N = [0, 1, 2, 4, 5, 6, 9, 10, 11]   # either side of every size guard of the stages
HINTS = [None, 0.0, 140.0]


def craft_random(n, seed):
    """Strictly increasing random indices, positive random env and floor."""
    rng = np.random.default_rng(1000 + seed)
    idx = np.cumsum(rng.integers(30, 400, size=n)).astype(np.int32)
    return idx, rng.uniform(0.05, 1.0, n), rng.uniform(0.01, 0.3, n)


def craft_beats(n, seed, sr=SR, doubled=0.04):
    """A heartbeat-like table: S1 peaks an RR of 0.8 s +- 10 % apart (a gap
    doubled now and then), an S2 0.3 s after most of them, weak peaks in
    between at times; cut to exactly n peaks."""
    rng = np.random.default_rng(2000 + seed)
    idx, env = [], []
    t = int(0.5 * sr)
    while len(idx) < n:
        idx.append(t)
        env.append(rng.uniform(0.8, 1.2))
        rr = int(round(0.8 * sr * rng.uniform(0.9, 1.1)))
        if rng.random() < doubled:
            rr *= 2
        if rng.random() < 0.85:
            idx.append(t + int(round(0.3 * sr * rng.uniform(0.9, 1.1))))
            env.append(rng.uniform(0.3, 0.7))
        if rng.random() < 0.25:
            idx.append(t + int(round(0.55 * sr)) + int(rng.integers(0, 12)))
            env.append(rng.uniform(0.12, 0.4))
        if rr > 1.5 * 0.8 * sr and rng.random() < 0.8:    # a pair of weak peaks somewhere inside a doubled gap
            c1 = t + int(round(rng.uniform(0.75, 1.2) * sr))
            idx.append(c1)
            env.append(rng.uniform(0.25, 0.9))
            idx.append(c1 + int(round(0.15 * sr)))
            env.append(rng.uniform(0.1, 0.2))
        t += rr
    idx = np.array(idx[:n], dtype=np.int32)
    assert n < 2 or np.all(np.diff(idx) > 0)
    return idx, np.array(env[:n]), rng.uniform(0.04, 0.1, n)


def craft(n, seed):
    return craft_random(n, seed) if n < 12 else craft_beats(n, seed, doubled=0.12)


def table(idx, env, flo, sr=SR, params=None, hint=None):
    return dict(idx=np.ascontiguousarray(idx, np.int32), env=np.ascontiguousarray(env, np.float64),
                flo=np.ascontiguousarray(flo, np.float64), sr=int(sr), params=params or PARAMS, hint=hint)


def from_full(inp, params, hint):
    """The packed form of a recording given as whole arrays."""
    pk = np.asarray(inp["peaks"], dtype=np.int64)
    env, flo = np.asarray(inp["env"], np.float64), np.asarray(getattr(inp["floor"], "values", inp["floor"]), np.float64)
    return table(pk, env[pk], flo[pk], inp["sr"], params, hint)


def host(t):
    """_host.beats_packed on a table: the comparison target."""
    n_env = int(t["idx"][-1]) + 1 if len(t["idx"]) else 0
    return H.beats_packed(t["idx"], t["env"], t["flo"], n_env, t["sr"], t["params"], t["hint"])


def assert_same(got, t, what="", curves="bits"):
    """``got``: dict(status, final_peaks, bpm_times, bpm, pass, tags) of the
    code under test.  Indices, tags, status and the pass values equal to the
    host library's; curves bit-identical (``curves="bits"``) or within TB.RTOL.
    Returns whether the curves were bit-identical."""
    want = host(t)
    n = len(t["idx"])
    if "error" in want:
        assert isinstance(want["error"], KeyError) and n < 2, what
        assert got["status"] == H.E_FEW_PEAKS, what
        assert len(got["final_peaks"]) == 0 and len(got["bpm"]) == 0, what
        assert np.array_equal(got["tags"], np.zeros(n, np.int8)), what      # the host labels them None as well
        return True
    assert got["status"] == H.OK, what
    assert np.array_equal(got["final_peaks"], want["final_peaks"]), what
    assert np.array_equal(got["tags"], want["tags"]), what
    ps = got["pass"]
    assert ps[0] == want["start_bpm"], what
    for v, k in ((ps[1], "peak_time"), (ps[2], "recovery_time")):
        assert (want[k] is None and v != v) or v == want[k], (what, k)
    assert len(got["bpm"]) == len(want["bpm"]) and len(got["bpm_times"]) == len(want["bpm_times"]), what
    bits = bool(np.array_equal(got["bpm_times"], want["bpm_times"], equal_nan=True) and
                np.array_equal(got["bpm"], want["bpm"], equal_nan=True))
    if curves == "bits":
        assert bits, what
    else:
        np.testing.assert_allclose(got["bpm_times"], want["bpm_times"], rtol=TB.RTOL, atol=0, equal_nan=True)
        np.testing.assert_allclose(got["bpm"], want["bpm"], rtol=TB.RTOL, atol=0, equal_nan=True)
    return bits


LABEL = {H.TAG_S1: B.S1_PAIRED, H.TAG_S2: B.S2_PAIRED, H.TAG_NOISE: "Noise"}


def assert_golden(got, g, what=""):
    """The bars of test_host_beats.py against the reference's own results:
    indices, pass values and labels exact, the curve to TB.RTOL."""
    if "error" in g:
        assert got["status"] == H.E_FEW_PEAKS, what
        return
    assert got["status"] == H.OK, what
    assert np.array_equal(got["final_peaks"], g["final_peaks"]), what
    ps = got["pass"]
    assert ps[0] == float(g["start_bpm"]), what
    for v, k in ((ps[1], "peak_time"), (ps[2], "recovery_time")):
        assert (np.isnan(g[k]) and v != v) or v == float(g[k]), (what, k)
    labels = dict(zip((int(k) for k in g["info_keys"]), (str(v).split("§")[0] for v in g["info_vals"])))
    for k, tg in zip(g["all_raw_peaks"], got["tags"]):
        want = labels[int(k)]
        if want in (B.LONE_S1, B.LONE_S1_LAST, B.LONE_S1_CASCADE):
            assert tg == H.TAG_LONE_S1, (what, k, want)
        elif want in (B.S1_GAP, B.S2_GAP):
            assert tg == H.TAG_NOISE, (what, k, want)          # gap corrections relabel Noise peaks
        else:
            assert LABEL[int(tg)] == want, (what, k, want)
    if "metrics" not in g:
        return
    np.testing.assert_allclose(got["bpm_times"], g["bpm_times"], rtol=TB.RTOL, atol=0)
    np.testing.assert_allclose(got["bpm"], g["bpm_v"], rtol=TB.RTOL, atol=0)


@functools.lru_cache(maxsize=None)
def golden_tables():
    """[(name, golden, table)] for TB.CASES, each with its own params and hint."""
    out = []
    for name in TB.CASES:
        g, params, hint, inp = TB.load_case(name)
        out.append((name, g, from_full(inp, params, hint)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_tables():
    """The oracle's hot path on synthetic recordings, as test_host_beats runs it."""
    from oracle import oracle as O
    out = []
    for seed in range(6):
        o = O.detect(O.synth(300 + seed, 44100 * (20 + 7 * seed), 44100, 1), 44100, PARAMS, mode="native")
        out.append((f"synth{300 + seed}", from_full(o, PARAMS, None)))
    return out


@functools.lru_cache(maxsize=None)
def crafted_tables():
    out = []
    for n in SMALL_N + [40, 300]:
        for h in HINTS:
            out.append((f"n{n}_hint{h}", table(*craft(n, n), hint=h)))
    idx, env, flo = craft(120, 7)
    out.append(("floor_above_env", table(idx, env, env + 0.25)))
    flo2 = flo.copy()
    flo2[::7] = np.nan
    out.append(("nan_floor", table(idx, env, flo2)))
    return out


@functools.lru_cache(maxsize=None)
def long_table(n=12000, seed=5):
    """About 12 000 peaks whose gap-fill and short-interval passes fire."""
    return table(*craft_beats(n, seed))


def refinement_fires(t):
    """(a Noise peak became a final beat: gap fill, a classified beat is not a
    final beat: rhythm / short-interval correction) by the host library."""
    r = host(t)
    fin = np.isin(t["idx"], r["final_peaks"])
    noise = r["tags"] == H.TAG_NOISE
    beat = (r["tags"] == H.TAG_S1) | (r["tags"] == H.TAG_LONE_S1)
    return bool((fin & noise).any()), bool((~fin & beat).any())


# ---- beats_core_driver's files ---------------------------------------------- #
def write_cases(path, tables):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(tables)))
        for t in tables:
            hint = float("nan") if t["hint"] is None else float(t["hint"])
            f.write(struct.pack("<iid", len(t["idx"]), t["sr"], hint))
            f.write(bytes(H.beat_params(t["params"])))
            f.write(t["idx"].tobytes() + t["env"].tobytes() + t["flo"].tobytes())


def read_results(path, tables):
    buf = open(path, "rb").read()
    o, out = 0, []
    for t in tables:
        status, nf, nb = struct.unpack_from("<iii", buf, o)
        o += 12
        ps = np.frombuffer(buf, np.float64, 3, o)
        o += 24
        fin = np.frombuffer(buf, np.int32, nf, o).astype(np.int64)
        o += 4 * nf
        bt = np.frombuffer(buf, np.float64, nb, o)
        o += 8 * nb
        bv = np.frombuffer(buf, np.float64, nb, o)
        o += 8 * nb
        n = len(t["idx"])
        tags = np.frombuffer(buf, np.int8, n, o)
        o += n
        out.append(dict(status=status, final_peaks=fin, bpm_times=bt, bpm=bv, **{"pass": ps}, tags=tags))
    assert o == len(buf)
    return out


assert ctypes.sizeof(H.BeatParams) == 33 * 8
