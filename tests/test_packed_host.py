"""The packed host path without a GPU: the native beat stage on per-peak
values (_host.beats_packed) against the same stage on whole arrays, the packed
form of beats.analyze_fast, engine.peak_capacity, and shard.run_sharded on a
CPU test double that offers run_host_packed."""
import functools

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import beats as B
from tests import goldens as G
from tests import test_beats as TB


@functools.lru_cache(maxsize=None)
def _case(name):
    g, params, hint, inp = TB.load_case(name)
    return params, hint, inp


def _packed(inp):
    """What engine.Packed.to_host hands over for a recording with these full arrays."""
    pk = np.asarray(inp["peaks"], dtype=np.int64)
    tr = np.asarray(inp["troughs"], dtype=np.int64)
    env, floor = np.asarray(inp["env"], dtype=np.float64), np.asarray(inp["floor"], dtype=np.float64)
    return dict(sr=inp["sr"], n_env=len(env), peaks=pk, env_pk=env[pk], floor_pk=floor[pk], troughs=tr,
                env_tr=env[tr], n_raw_troughs=0, flags=0)


def _same_result(a, b):
    assert ("error" in a) == ("error" in b)
    if "error" in a:
        assert type(a["error"]) is type(b["error"]) is KeyError and a["error"].args == b["error"].args
        return
    assert sorted(a) == sorted(b)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v, b[k], equal_nan=v.dtype.kind == "f"), k
        else:
            assert v == b[k], k


@pytest.mark.parametrize("name", TB.CASES)
def test_beats_packed_equals_beats(name):
    params, hint, inp = _case(name)
    full = H.beats(inp["env"], inp["sr"], inp["floor"], inp["peaks"], params, hint)
    p = _packed(inp)
    got = H.beats_packed(p["peaks"], p["env_pk"], p["floor_pk"], p["n_env"], p["sr"], params, hint)
    _same_result(got, full)
    assert H.packed_scratch_is_nan()


def test_error_cases_are_covered():
    """The comparison above includes recordings the stage refuses (< 2 raw peaks)."""
    errs = [n for n in TB.CASES if "error" in H.beats(*(_case(n)[2][k] for k in ("env", "sr", "floor", "peaks")),
                                                       _case(n)[0], _case(n)[1])]
    assert errs


def test_scratch_reuse_on_one_thread():
    """A long recording, a short one, the long one again on the same scratch:
    nothing of one call is left for the next."""
    runs = []
    for name in ("vulpine", "ref_44k_short16", "vulpine", "ref_44k_10s_zeros", "vulpine"):
        params, hint, inp = _case(name)
        p = _packed(inp)
        r = H.beats_packed(p["peaks"], p["env_pk"], p["floor_pk"], p["n_env"], p["sr"], params, hint)
        assert H.packed_scratch_is_nan(), name
        _same_result(r, H.beats(inp["env"], inp["sr"], inp["floor"], inp["peaks"], params, hint))
        runs.append(r)
    _same_result(runs[0], runs[2])
    _same_result(runs[0], runs[4])
    assert len(_case("vulpine")[2]["env"]) > len(_case("ref_44k_short16")[2]["env"])


def test_beats_packed_rejects_bad_input():
    with pytest.raises(ValueError):
        H.beats_packed([3, 40], [1.0, 2.0], [0.5, 0.5], 40, 302, _case("vulpine")[0])
    with pytest.raises(ValueError):
        H.beats_packed([3, 20], [1.0], [0.5, 0.5], 40, 302, _case("vulpine")[0])
    assert H.packed_scratch_is_nan()


def test_analyze_fast_on_packed_dicts():
    names = ["ref_44k_60s_mono", "ref_44k_40s_clicks", "ref_44k_10s_zeros", "vulpine", "ref_44k_short16"]
    params = _case(names[0])[0]
    full = [dict(_case(n)[2]) for n in names]
    packed = [_packed(r) for r in full]
    want = B.analyze_fast(full, params)
    seq = B.analyze_fast(packed, params)
    thr = B.analyze_fast(packed, params, threads=3)
    assert len(want) == len(seq) == len(thr) == len(names)
    for w, s, t in zip(want, seq, thr):
        _same_result(s, w)
        _same_result(t, s)
    mixed = B.analyze_fast([packed[0], full[1], {"error": ValueError("x")}], params, threads=2)
    _same_result(mixed[0], want[0])
    _same_result(mixed[1], want[1])
    assert isinstance(mixed[2]["error"], ValueError)


@pytest.mark.parametrize("nd,distance,want", [(1, 1, 1), (16, 30, 1), (18124, 30, 605), (0, 5, 0)])
def test_peak_capacity_by_hand(nd, distance, want):
    from bpm_analysis_amd.engine import peak_capacity
    assert peak_capacity(nd, distance) == want


@pytest.mark.parametrize("name", G.names(kind="env"))
def test_peak_capacity_bounds_the_oracle(name):
    from bpm_analysis_amd.engine import peak_capacity
    from oracle import oracle as O
    g = G.load(name)
    env = g["env"]
    if len(env) <= 15:
        return
    d = G.env_derived(g)
    cap = peak_capacity(len(env), d.distance)
    floor, troughs, _ = O.noise_floor(env, d, g["params"])
    peaks = O.raw_peaks(env, floor, d, g["params"])
    assert cap >= len(peaks) and cap >= len(troughs)
    assert cap >= len(g["peaks"]) and cap >= len(g["troughs"])     # the reference's own counts
    raw = O.find_peaks(env, distance=d.distance, negate=True,
                       prominence=O.quantile(env, g["params"]["trough_prominence_quantile"]))
    assert cap >= len(raw)                                         # a static floor keeps the raw troughs


class _FullDouble:
    """engine.Detector's host entry point on the CPU: the oracle computes the hot path."""

    def __init__(self):
        import torch
        self.device = torch.device("cpu")
        self.calls = []

    def _detect(self, recs, fs, params, mode):
        from oracle import oracle as O
        ds = O.derive(fs, params).ds
        return [None if -(-len(r) // ds) <= 15 else O.detect(r, fs, params, mode=mode) for r in recs]

    def run_host(self, recs, fs, params, mode="native", stages=7, resolve_ties=False):
        self.calls.append("full")
        return [{"flags": 8} if o is None else {k: o[k] for k in ("env", "floor", "troughs", "peaks", "sr", "flags")}
                for o in self._detect(recs, fs, params, mode)]


class _PackedDouble(_FullDouble):
    def run_host_packed(self, recs, fs, params, mode="native", stages=7, resolve_ties=False, want_y16=False,
                        longest_first=True):
        self.calls.append("packed")
        out = []
        for o in self._detect(recs, fs, params, mode):
            if o is None:
                z = np.zeros(0)
                out.append(dict(sr=0, n_env=0, peaks=z.astype(np.int64), env_pk=z, floor_pk=z,
                                troughs=z.astype(np.int64), env_tr=z, n_raw_troughs=0, flags=8))
                continue
            out.append(dict(_packed(o), flags=o["flags"]))
        return out


@pytest.mark.parametrize("beats", ["native", False, "python"])
def test_run_sharded_takes_the_packed_entry_point(beats):
    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd.shard import run_sharded
    from oracle import oracle as O
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    items = [O.synth(60 + i, n, 44100, 1) for i, n in enumerate([44100 * 9, 44100 * 14 + 3, 146 * 15, 44100 * 11])]
    full, packed, off = _FullDouble(), _PackedDouble(), _PackedDouble()
    kw = dict(fs=44100, mode="native", beats=beats, host_threads=2, chunk_frames=44100 * 20)
    a = run_sharded(items, params, detector=full, **kw)
    b = run_sharded(items, params, detector=packed, **kw)
    c = run_sharded(items, params, detector=off, packed=False, **kw)
    assert set(full.calls) == {"full"} and set(off.calls) == {"full"}
    assert set(packed.calls) == ({"full"} if beats == "python" else {"packed"})
    assert len(a) == len(b) == len(c) == len(items)
    for x, y, z in zip(a, b, c):
        assert sorted(x) == sorted(y) == sorted(z)
        for k, v in x.items():
            if k == "error":
                assert type(v) is type(y[k]) is type(z[k]) and str(v) == str(y[k]) == str(z[k])
            elif isinstance(v, np.ndarray):
                assert v.dtype == y[k].dtype and np.array_equal(v, y[k]) and np.array_equal(v, z[k]), k
            else:
                assert v == y[k] == z[k], k
    assert isinstance(a[2]["error"], ValueError) and "padlen" in str(a[2]["error"])
    assert len(a[0]["raw_peaks"]) > 5
    if beats:
        assert len(a[0]["final_peaks"]) > 2 and len(a[0]["bpm"]) > 2
