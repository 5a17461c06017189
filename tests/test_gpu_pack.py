"""bpmx_pack on the GPU: the ragged per-peak / per-trough tables and the int16
debug samples against numpy on crafted inputs (the kernels apart from the
pipeline), then through the pipeline, the tie resolution, the drop-in's debug
WAVs and the sharded runner."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import goldens as G

pytestmark = pytest.mark.gpu

SENT_I, SENT_F, SENT_O, SENT_16 = -7, 123.456, -99, 0x5A5A


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(det, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(det.device)


# ------------------------------------------------------------------ crafted tables
DIST = 5


def _crafted(det, F, seed, zero_all=False):
    """A Result filled by hand (ds = 1): random lengths, counts up to the
    capacity with empty files at both ends and in a run, sorted distinct
    indices, env / floor with NaN, inf and -0.0 among the values."""
    from bpm_analysis_amd.engine import peak_capacity
    rng = np.random.default_rng(seed)
    nd = rng.integers(16, 401, size=F)
    fo = np.zeros(F + 1, dtype=np.int64)
    fo[1:] = np.cumsum(nd)
    tot = int(fo[-1])
    env, floor = rng.normal(size=tot), rng.normal(size=tot)
    for arr in (env, floor):
        pos = rng.choice(tot, size=max(tot // 6, 3), replace=False)
        arr[pos] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0]), size=len(pos))
        arr[rng.choice(tot, size=3, replace=False)] = np.array([0x7ff8dead0000beef, 0xfff0000000000001,
                                                                0x8000000000000000], dtype=np.uint64).view(np.float64)
    res = det.alloc(fo, 1, 302)
    cnt = {}
    idx = {}
    for w in ("peaks", "troughs"):
        c = np.array([rng.integers(0, peak_capacity(n, DIST) + 1) for n in nd], dtype=np.int32)
        if F >= 3:
            c[0] = c[-1] = 0
        if F >= 20:
            c[7:12] = 0
        if zero_all:
            c[:] = 0
        full = rng.integers(0, 1 << 40, size=tot).astype(np.int64)      # beyond the counts: never read as indices
        for f in range(F):
            full[fo[f]:fo[f] + c[f]] = np.sort(rng.choice(nd[f], size=c[f], replace=False))
        cnt[w], idx[w] = c, full
    res.env.copy_(_dev(det, env))
    res.floor.copy_(_dev(det, floor))
    res.peaks.copy_(_dev(det, idx["peaks"]))
    res.troughs.copy_(_dev(det, idx["troughs"]))
    res.n_peaks.copy_(_dev(det, cnt["peaks"]))
    res.n_troughs.copy_(_dev(det, cnt["troughs"]))
    want = {}
    for w, vals in (("peaks", (env, floor)), ("troughs", (env,))):
        off = np.zeros(F + 1, dtype=np.int64)
        off[1:] = np.cumsum(cnt[w])
        i = np.concatenate([idx[w][fo[f]:fo[f] + cnt[w][f]] for f in range(F)] + [np.zeros(0, np.int64)])
        base = np.repeat(fo[:-1], cnt[w])
        want[w] = (off, i.astype(np.int32), [_u64(v[base + i]) for v in vals])
    return res, want


def _fill_sentinels(q):
    q.pk_off.fill_(SENT_O); q.tr_off.fill_(SENT_O)
    q.pk_idx.fill_(SENT_I); q.tr_idx.fill_(SENT_I)
    q.pk_env.fill_(SENT_F); q.pk_floor.fill_(SENT_F); q.tr_env.fill_(SENT_F)


def _check_tables(q, want, cap_p, cap_t):
    """Offsets are the true prefix sums; entries below min(total, cap) are the
    numpy gather's; everything from there on is the sentinel."""
    h = lambda t: t.cpu().numpy()
    for w, off_t, idx_t, val_ts, cap in (("peaks", q.pk_off, q.pk_idx, (q.pk_env, q.pk_floor), cap_p),
                                         ("troughs", q.tr_off, q.tr_idx, (q.tr_env,), cap_t)):
        off, i, vals = want[w]
        assert np.array_equal(h(off_t), off), w
        n = min(int(off[-1]), cap)
        got_i = h(idx_t)
        assert np.array_equal(got_i[:n], i[:n]), w
        assert (got_i[n:] == SENT_I).all(), w
        for t, v in zip(val_ts, vals):
            g = _u64(h(t))
            assert np.array_equal(g[:n], v[:n]), w
            assert (g[n:] == _u64(np.array([SENT_F]))[0]).all(), w


@pytest.mark.parametrize("F,zero_all", [(1, False), (1, True), (3, False), (1300, False)])
def test_gather_on_crafted_inputs(det, F, zero_all):
    res, want = _crafted(det, F, seed=100 + F, zero_all=zero_all)
    q = det.alloc_packed(res, DIST)
    _fill_sentinels(q)
    assert det.pack(res, DIST, out=q) is q
    assert q.cap_peaks >= int(want["peaks"][0][-1]) and q.cap_troughs >= int(want["troughs"][0][-1])
    _check_tables(q, want, q.cap_peaks, q.cap_troughs)
    if not zero_all and F > 1:
        assert int(want["peaks"][0][-1]) > 0 and int(want["troughs"][0][-1]) > 0
    # the host view of the same tables
    host = q.to_host()
    nd = np.diff(res.doff)
    for f in (0, F // 2, F - 1):
        off, i, vals = want["peaks"]
        a, b = int(off[f]), int(off[f + 1])
        r = host[f]
        assert r["n_env"] == nd[f] and r["peaks"].dtype == np.int64 and np.array_equal(r["peaks"], i[a:b])
        assert np.array_equal(_u64(r["env_pk"]), vals[0][a:b]) and np.array_equal(_u64(r["floor_pk"]), vals[1][a:b])
        off, i, vals = want["troughs"]
        a, b = int(off[f]), int(off[f + 1])
        assert np.array_equal(r["troughs"], i[a:b]) and np.array_equal(_u64(r["env_tr"]), vals[0][a:b])


@pytest.mark.parametrize("F", [3, 1300])
@pytest.mark.parametrize("short", ["one", "all"])
def test_overflow_leaves_totals_and_writes_nothing_beyond_cap(det, F, short):
    from bpm_analysis_amd import _native as N
    res, want = _crafted(det, F, seed=100 + F)
    tp, tt = int(want["peaks"][0][-1]), int(want["troughs"][0][-1])
    assert tp > 1 and tt > 1
    cap_p, cap_t = (tp - 1, tt - 1) if short == "one" else (0, 0)
    q = det.alloc_packed(res, DIST)           # tensors longer than the capacities in force
    q.cap_peaks, q.cap_troughs = cap_p, cap_t
    _fill_sentinels(q)
    with pytest.raises(N.BpmxError) as e:
        det.pack(res, DIST, out=q)
    assert e.value.code == N.E_LIMIT
    _check_tables(q, want, cap_p, cap_t)
    with pytest.raises(N.BpmxError) as e:
        q.to_host()
    assert e.value.code == N.E_LIMIT
    # one table short is enough
    q2 = det.alloc_packed(res, DIST, cap_troughs=tt - 1)
    with pytest.raises(N.BpmxError) as e:
        det.pack(res, DIST, out=q2)
    assert e.value.code == N.E_LIMIT


# ------------------------------------------------------------------ pipeline
FS = 44100
LENS = [FS * 3, 146 * 15, FS * 20, FS * 7 + 5, FS * 1]


@pytest.fixture(scope="module")
def recs():
    return [O.synth(500 + i, n, FS, 1) for i, n in enumerate(LENS)]


@pytest.mark.parametrize("mode", ["reference", "native"])
def test_run_host_packed_equals_run_host(det, recs, mode):
    from bpm_analysis_amd import _native as N
    params = dict(G.BASE_PARAMS)
    full = det.run_host(recs, FS, params, mode=mode, want_y=True)
    packed = det.run_host_packed(recs, FS, params, mode=mode, want_y16=True)
    assert len(full) == len(packed) == len(recs)
    for f, (a, p) in enumerate(zip(full, packed)):
        assert p["flags"] == a["flags"] and p["n_raw_troughs"] == a["n_raw_troughs"] and p["sr"] == a["sr"]
        assert p["n_env"] == len(a["env"])
        assert p["peaks"].dtype == np.int64 and np.array_equal(p["peaks"], a["peaks"])
        assert p["troughs"].dtype == np.int64 and np.array_equal(p["troughs"], a["troughs"])
        assert np.array_equal(_u64(p["env_pk"]), _u64(a["env"][a["peaks"]]))
        assert np.array_equal(_u64(p["floor_pk"]), _u64(a["floor"][a["peaks"]]))
        assert np.array_equal(_u64(p["env_tr"]), _u64(a["env"][a["troughs"]]))
        if f == 1:
            assert a["flags"] & N.F_TOO_SHORT
            for k in ("peaks", "env_pk", "floor_pk", "troughs", "env_tr", "y16"):
                assert len(p[k]) == 0, k
            assert p["n_env"] == 0
            continue
        assert len(p["peaks"]) > 2 and len(p["troughs"]) > 2
        y = a["y"]
        assert p["y16"].dtype == np.int16 and np.array_equal(p["y16"], np.int16(y / np.max(np.abs(y)) * 32767))
        assert p["y_max"] == np.max(np.abs(y))
    o = O.detect(recs[3], FS, params, mode=mode)
    p = packed[3]
    assert np.array_equal(p["peaks"], o["peaks"]) and np.array_equal(p["troughs"], o["troughs"])
    if mode == "reference":
        assert np.array_equal(_u64(p["env_pk"]), _u64(o["env"][o["peaks"]]))
        assert np.array_equal(_u64(p["floor_pk"]), _u64(o["floor"][o["peaks"]]))
    # without the debug samples nothing of them is returned
    assert "y16" not in det.run_host_packed(recs[:1], FS, params, mode=mode)[0]


@pytest.mark.parametrize("name", G.names(kind="env", prefix="env_ties"))
def test_pack_sees_the_resolved_ties(det, name):
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd.design import detect_design
    g = G.load(name)
    sr, env = int(g["sr"]), np.ascontiguousarray(g["env"], dtype=np.float64)
    fo = np.array([0, len(env)], dtype=np.int64)
    d = detect_design(sr, g["params"])
    st = N.STAGE_FLOOR | N.STAGE_PEAKS
    res = det.alloc(fo, 1, sr)
    res.env.copy_(_dev(det, env))
    det.run(None, fo, sr, g["params"], stages=st, out=res, d=d)
    before = res.to_host()[0]
    assert before["flags"] & (N.F_TROUGH_TIE | N.F_PEAK_TIE)
    assert det.resolve_ties(res, g["params"], st) == 1
    p = det.pack(res, d.distance).to_host()[0]
    a = res.to_host()[0]
    assert a["flags"] & (N.F_TROUGH_ORDERED | N.F_PEAK_ORDERED) and not a["flags"] & (N.F_TROUGH_TIE | N.F_PEAK_TIE)
    assert p["flags"] == a["flags"] and p["n_raw_troughs"] == a["n_raw_troughs"] and p["n_env"] == len(env)
    assert np.array_equal(p["peaks"], a["peaks"]) and np.array_equal(p["troughs"], a["troughs"])
    assert np.array_equal(_u64(p["env_pk"]), _u64(a["env"][a["peaks"]]))
    assert np.array_equal(_u64(p["floor_pk"]), _u64(a["floor"][a["peaks"]]))
    assert np.array_equal(_u64(p["env_tr"]), _u64(a["env"][a["troughs"]]))


# ------------------------------------------------------------------ y16
Y_LENS = [1, 2, 63, 64, 65, 4099]
Y_KINDS = ["random", "max_first", "max_last", "neg_max", "plus_minus", "denormal", "zeros", "nan", "inf"]


def _y_file(kind, n, rng):
    y = rng.normal(size=n)
    if kind == "max_first":
        y[0] = 10.0
    elif kind == "max_last":
        y[-1] = 10.0
    elif kind == "neg_max":
        y[n // 2] = -10.0
    elif kind == "plus_minus":
        y[-1] = -7.5
        y[0] = 7.5
    elif kind == "denormal":
        y = (rng.integers(1, 1000, size=n) * rng.choice([-1, 1], size=n)) * 5e-324
        assert np.all(np.abs(y) < 2.3e-308) and np.all(y != 0)
    elif kind == "zeros":
        y = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    elif kind == "nan":
        y[n // 3] = np.nan
    elif kind == "inf":
        y[n // 2] = -np.inf if n % 2 else np.inf
    return y


@pytest.mark.parametrize("lead", [3, 4])
def test_y16_on_crafted_signals(det, lead):
    """Every kind of content at every length, back to back (so slices start at
    odd and even offsets), in a y16 buffer that starts `lead` elements into a
    larger one: both 4-byte phases of the base, guard elements on both sides."""
    import torch
    rng = np.random.default_rng(77)
    files = [(k, n) for n in Y_LENS for k in Y_KINDS]
    ys = [_y_file(k, n, rng) for k, n in files]
    fo = np.zeros(len(ys) + 1, dtype=np.int64)
    fo[1:] = np.cumsum([len(y) for y in ys])
    tot = int(fo[-1])
    assert any(int(a) % 2 for a in fo[:-1]) and any(int(a) % 2 == 0 for a in fo[1:-1])
    res = det.alloc(fo, 1, 302, want_y=True)
    res.y.copy_(_dev(det, np.concatenate(ys)))
    q = det.alloc_packed(res, 1, want_y16=True)
    big = torch.full((tot + 16,), SENT_16, dtype=torch.int16, device=det.device)
    q.y16 = big[lead:lead + tot]
    q.y_max.fill_(-1.0)
    det.pack(res, 1, want_y16=True, out=q)
    got = big.cpu().numpy()
    assert (got[:lead] == SENT_16).all() and (got[lead + tot:] == SENT_16).all()
    ymax = q.y_max.cpu().numpy()
    host = q.to_host()
    for f, ((kind, n), y) in enumerate(zip(files, ys)):
        m = np.max(np.abs(y))
        assert _u64(ymax[f:f + 1])[0] == _u64(np.array([m]))[0], (kind, n)
        if kind in ("zeros", "nan", "inf"):
            want = np.zeros(n, dtype=np.int16)
        else:
            assert np.isfinite(m) and m > 0
            want = np.int16(y / np.max(np.abs(y)) * 32767)
        g = got[lead + fo[f]:lead + fo[f + 1]]
        assert np.array_equal(g, want), (kind, n)
        assert np.array_equal(host[f]["y16"], want)
        if kind == "plus_minus":
            assert g[0] == 32767 and (n == 1 or g[-1] == -32767)
        if kind == "neg_max":
            assert g[n // 2] == -32767


# ------------------------------------------------------------------ consumers
def _two_wavs(tmp_path):
    from scipy.io import wavfile
    paths = []
    for i, n in enumerate([FS * 6 + 1, FS * 9]):
        paths.append(str(tmp_path / f"rec{i}.wav"))
        wavfile.write(paths[-1], FS, O.synth(700 + i, n, FS, 1))
    return paths


def test_native_mode_debug_wavs_come_from_y16(det, tmp_path):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin
    params = dict(G.BASE_PARAMS, save_filtered_wav=True)
    paths = _two_wavs(tmp_path)
    outdir = tmp_path / "out"
    outdir.mkdir()
    res = dropin.analyze_wav_files(paths, params, str(outdir), mode="native")
    full = det.run_host([wavfile.read(p)[1] for p in paths], FS, params, mode="native", want_y=True,
                        resolve_ties=True)
    for path, r, a in zip(paths, res, full):
        assert "error" not in r
        assert np.array_equal(r["env"], a["env"]) and np.array_equal(r["peaks"], a["peaks"])
        want = np.int16(a["y"] / np.max(np.abs(a["y"])) * 32767)
        name = path.split("/")[-1][:-4] + "_filtered_debug.wav"
        for dbg in (path[:-4] + "_filtered_debug.wav", str(outdir / name)):
            sr, got = wavfile.read(dbg)
            assert sr == a["sr"] and got.dtype == np.int16 and np.array_equal(got, want)


def test_run_sharded_never_downloads_whole_arrays(det, tmp_path, monkeypatch):
    from bpm_analysis_amd import engine
    from bpm_analysis_amd.shard import run_sharded
    from bpm_analysis_amd import DEFAULT_PARAMS
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    paths = _two_wavs(tmp_path)
    want = run_sharded(paths, params, mode="native", beats="native", detector=det, host_threads=2, packed=False)

    def boom(self):
        raise AssertionError("Result.to_host called on the packed path")

    monkeypatch.setattr(engine.Result, "to_host", boom)
    got = run_sharded(paths, params, mode="native", beats="native", detector=det, host_threads=2)
    assert len(got) == len(want) == 2
    assert len(got[1]["final_peaks"]) > 2 and len(got[1]["bpm"]) > 2
    for g, w in zip(got, want):
        assert "error" not in g and sorted(g) == sorted(w)
        assert len(g["raw_peaks"]) > 5
        for k, v in w.items():
            if isinstance(v, np.ndarray):
                assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k
            else:
                assert v == g[k], k
