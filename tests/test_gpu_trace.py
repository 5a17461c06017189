"""bpmx_beats_device_ex (k_beats_trace / k_beats_hints) and
bpmx_pack_trough_floor on the MI355X.  The trace is compared bit for bit with
tests/trace_core_driver.cpp (the same text on the CPU) as whole slices, so
what the kernel must leave alone is compared as well: every output is filled
with sentinels first (the trace with 0xFF bytes, as the driver fills its own).
Everything is compared for equality."""
import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from tests import beats_cases as C
from tests import test_beats as TB
from tests import test_gpu_beats as G
from tests import trace_cases as T

pytestmark = pytest.mark.gpu

COUNTS = [0, 0, 1, 2, 5, 6, 9, 10, 11, 0, 63, 64, 65, 230, 605, 40, 0, 17, 128, 300, 12, 0, 0]
RESULTS = ("final_idx", "n_final", "bpm_t", "bpm", "n_bpm", "pass_", "tags", "status")
PAD = 8                                               # elements kept beyond every capacity


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    """tables -> (results, whole trace slices) of trace_core_driver."""
    work = tmp_path_factory.mktemp("gpu_trace")
    exe = str(work / "trace_core_driver")
    b = T.build_driver(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    count = [0]

    def run(tables):
        count[0] += 1
        base = str(work / f"c{count[0]}")
        C.write_cases(base + ".in", tables)
        return T.run_driver(exe, base + ".in", base + ".out", base + ".tr", tables)

    return run


def _run(det, pk, params, hint=None, hints=None, trace=True):
    """bpmx_beats_device_ex with every output filled with sentinels first -> host arrays."""
    import torch
    F, cap, dev = pk.n_files, max(int(pk.cap_peaks), 1), det.device
    full = lambda n, v, dt: torch.full((n + PAD,), v, dtype=dt, device=dev)  # noqa: E731
    ones = lambda n, dt: torch.full((n + PAD,), -1, dtype=torch.int64 if dt == torch.float64 else dt,  # noqa: E731
                                    device=dev).view(dt)
    out = dict(final_idx=full(cap, G.I32_S, torch.int32), n_final=full(F, G.I32_S, torch.int32),
               bpm_t=full(cap, G.F64_S, torch.float64), bpm=full(cap, G.F64_S, torch.float64),
               n_bpm=full(F, G.I32_S, torch.int32), pass_=full(3 * F, G.F64_S, torch.float64),
               tags=full(cap, G.I8_S, torch.int8), status=full(F, G.I32_S, torch.int32))
    tr = dict(record=ones(cap * N.TR_NFIELDS, torch.float64), code=ones(cap, torch.int32),
              lt_pos=ones(cap, torch.int32), lt_bpm=ones(cap, torch.float64), n_lt=ones(F, torch.int32),
              dev_t=ones(cap, torch.float64), dev=ones(cap, torch.float64), gap=ones(cap, torch.int32))
    bp = H.beat_params(params)
    k = N.PackedOut()
    k.cap_peaks = pk.cap_peaks
    k.pk_off, k.pk_idx = pk.pk_off.data_ptr(), pk.pk_idx.data_ptr()
    k.pk_env, k.pk_floor = pk.pk_env.data_ptr(), pk.pk_floor.data_ptr()
    o = N.BeatsOut()
    for name, _ in N.BeatsOut._fields_:
        setattr(o, name, out[name].data_ptr())
    t = N.TraceOut()
    for name, _ in N.TraceOut._fields_:
        setattr(t, name, tr[name].data_ptr())
    d_hints = None
    if hints is not None:
        d_hints = torch.from_numpy(np.array([np.nan if h is None else h for h in hints], np.float64)).to(dev)
    N.check(det.L.bpmx_beats_device_ex(det.ctx, F, int(pk.sr), ctypes.byref(bp),
                                       float("nan") if hint is None else float(hint), ctypes.byref(k),
                                       None if pk.flags is None else pk.flags.data_ptr(), ctypes.byref(o),
                                       None if d_hints is None else d_hints.data_ptr(),
                                       ctypes.byref(t) if trace else None, det.stream_handle()),
            "bpmx_beats_device_ex")
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in out.items()}, {k_: v.cpu().numpy() for k_, v in tr.items()}


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check_trace(tr, tables, off, want, cap=None, dead=()):
    """Every file's slices against the driver's, everything no live file owns
    against 0xFF (files in `dead`, or beyond `cap`, own nothing)."""
    F = len(tables)
    cap = int(off[-1]) if cap is None else cap
    owned = {k: np.zeros(len(tr[k]), bool) for k, _, _ in T.SLICES}
    for f, (t, w) in enumerate(zip(tables, want)):
        a, n = int(off[f]), len(t["idx"])
        if f in dead or a + n > cap:
            assert _untouched(tr["n_lt"][f:f + 1]), f
            continue
        assert int(tr["n_lt"][f]) == w["n_lt"], f
        for k, _, per in T.SLICES:
            got = tr[k][a * per:(a + n) * per]
            assert got.tobytes() == w[k].tobytes(), (f, n, k)
            owned[k][a * per:(a + n) * per] = True
    for k, _, _ in T.SLICES:
        assert _untouched(tr[k][~owned[k]]), f"{k}: a write outside the files' slices"
    assert _untouched(tr["n_lt"][F:])


def _tables(counts=COUNTS, hint=None):
    return [C.table(*C.craft(n, 50 + f), hint=hint) for f, n in enumerate(counts)]


def _same_results(a, b):
    for k in RESULTS:
        assert a[k].tobytes() == b[k].tobytes(), k


def _trace_and_plain(det, cpu, tables, hint=None):
    pk = G._upload(det, tables)
    off = G._offsets(tables)
    res, tr = _run(det, pk, C.PARAMS, hint)
    _, want = cpu(tables)
    _check_trace(tr, tables, off, want)
    plain = G._run(det, pk, C.PARAMS, hint)
    for k in RESULTS:                                 # G._run keeps the same 8 spare elements
        assert res[k].tobytes() == plain[k].tobytes(), k
    G._check_batch(res, tables, off)
    return res, tr


# ---- 1. crafted batches ----------------------------------------------------------- #
@pytest.mark.parametrize("hint", C.HINTS)
def test_crafted_batch(det, cpu, hint):
    assert len(COUNTS) == 23 and COUNTS[0] == COUNTS[-1] == 0
    _trace_and_plain(det, cpu, _tables(hint=hint), hint)


def test_single_file(det, cpu):
    _trace_and_plain(det, cpu, [C.table(*C.craft(300, 62))])


def test_global_workspace_gives_the_same(det, cpu):
    tables = _tables()
    a = _trace_and_plain(det, cpu, tables)
    det.set_options(N.OPT_BEATS_GLOBAL)
    try:
        b = _trace_and_plain(det, cpu, tables)
    finally:
        det.set_options(0)
    for x, y in zip(a, b):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


def test_first_table_past_the_lds_limit(det, cpu):
    t = C.table(*C.craft(689, 3))
    assert len(t["idx"]) > 688                        # beyond the LDS budget (bpmx_plan.h)
    _trace_and_plain(det, cpu, [t])


def test_long_table_with_gap_fill(det, cpu):
    t = C.long_table()
    assert C.refinement_fires(t)[0]
    _, tr = _trace_and_plain(det, cpu, [t])
    assert (tr["gap"][:len(t["idx"])] != 0).any()     # the gap history holds labels


# ---- 2. overflow and skip ---------------------------------------------------------- #
def test_capacity_smaller_than_the_total(det, cpu):
    tables = _tables()
    off = G._offsets(tables)
    cap = int(off[13]) + 20                           # file 13 (230 peaks) straddles it
    assert off[13] < cap < off[14]
    res, tr = _run(det, G._upload(det, tables, cap=cap), C.PARAMS)
    _, want = cpu(tables)
    G._check_batch(res, tables, off, cap=cap)
    _check_trace(tr, tables, off, want, cap=cap)
    st = res["status"][:len(tables)]
    assert (st[13:] == N.BEATS_OVERFLOW).all() and (st[:13] != N.BEATS_OVERFLOW).all()


def test_flagged_file_is_skipped(det, cpu):
    tables = _tables()
    flags = np.zeros(len(tables), np.int32)
    flags[13] = N.F_TOO_SHORT
    flags[10] = N.F_STATIC_FLOOR                      # an informative bit skips nothing
    res, tr = _run(det, G._upload(det, tables, flags=flags), C.PARAMS)
    _, want = cpu(tables)
    G._check_batch(res, tables, G._offsets(tables), skipped={13})
    _check_trace(tr, tables, G._offsets(tables), want, dead={13})
    assert res["status"][13] == N.BEATS_SKIPPED


# ---- 3. per-file hints --------------------------------------------------------------- #
HINTS8 = [None, 0, 40, 80, 140, 220, None, 60]


@pytest.mark.parametrize("trace", [True, False])
def test_hints_per_file_in_one_launch(det, cpu, trace):
    tables = [C.table(*C.craft(120, 70 + f), hint=h) for f, h in enumerate(HINTS8)]
    off = G._offsets(tables)
    res, tr = _run(det, G._upload(det, tables), C.PARAMS, hint=111.0, hints=HINTS8, trace=trace)
    want_res, want = cpu(tables)                      # eight runs, each with its scalar hint
    G._check_batch(res, tables, off)
    for f, w in enumerate(want_res):
        a, nf = int(off[f]), int(res["n_final"][f])
        assert np.array_equal(res["final_idx"][a:a + nf], w["final_peaks"]), f
        assert res["pass_"][3 * f:3 * f + 3].tobytes() == w["pass"].tobytes(), f
    assert len({float(res["pass_"][3 * f]) for f in range(8)}) > 3       # the hints took effect
    if trace:
        _check_trace(tr, tables, off, want)
    else:
        assert all(_untouched(v) for v in tr.values())


# ---- 4. the goldens as batches -------------------------------------------------------- #
def test_golden_strings_from_the_device(det):
    from bpm_analysis_amd import explain as X
    gold = [(n, g, t) for n, g, t in C.golden_tables() if "info_vals" in g]
    assert len(gold) == 26
    groups = {}
    for name, g, t in gold:
        groups.setdefault((bytes(H.beat_params(t["params"])), t["hint"], t["sr"]), []).append((name, g, t))
    for members in groups.values():
        tables = [t for _, _, t in members]
        off = G._offsets(tables)
        res, tr = _run(det, G._upload(det, tables), tables[0]["params"], tables[0]["hint"])
        for f, (name, g, t) in enumerate(members):
            a, n = int(off[f]), len(t["idx"])
            one = {k: tr[k][a * per:(a + n) * per] for k, _, per in T.SLICES}
            one["n_lt"] = int(tr["n_lt"][f])
            data = X.assemble(t["idx"], t["sr"], t["params"], T.used(one, n))
            want = dict(zip((int(k) for k in g["info_keys"]), (str(v) for v in g["info_vals"])))
            assert {int(k): v for k, v in data["beat_debug_info"].items()} == want, name
            lt = data["long_term_bpm_series"]
            assert np.asarray(lt.values).tobytes() == np.asarray(g["lt_v"], np.float64).tobytes(), name
            assert np.asarray(lt.index).tobytes() == np.asarray(g["lt_t"], np.float64).tobytes(), name
            assert np.asarray(data["deviation_series"].values).tobytes() == \
                np.asarray(g["dev_v"], np.float64).tobytes(), name


# ---- 5. the floor at the troughs ------------------------------------------------------- #
@pytest.mark.parametrize("short", [False, True])
def test_trough_floor_gather(det, short):
    import torch
    nd = [16, 1000, 18124, 16, 4000]
    rng = np.random.default_rng(9)
    doff = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    floor = rng.uniform(0.01, 1.0, int(doff[-1]))
    cnt = [0, 37, 700, 3, 0]
    idx = [np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for n, c in zip(nd, cnt)]
    tr_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    tr_idx = np.concatenate(idx)
    special = np.array([0x7FF8000000ABCDEF, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
    for j, bits in zip((0, 5, 40, 736), special):     # a NaN with a payload, -0.0, +inf, -inf at trough positions
        f = int(np.searchsorted(tr_off, j, side="right") - 1)
        floor.view(np.uint64)[doff[f] + tr_idx[j]] = bits
    tot = int(tr_off[-1])
    cap = tot - 100 if short else tot
    dev = det.device
    d_floor = torch.from_numpy(floor).to(dev)
    d_off, d_idx = torch.from_numpy(tr_off).to(dev), torch.from_numpy(tr_idx).to(dev)
    out = torch.full((tot + PAD,), -1, dtype=torch.int64, device=dev)
    o = N.Out()
    o.floor = d_floor.data_ptr()
    k = N.PackedOut()
    k.cap_troughs, k.tr_off, k.tr_idx = cap, d_off.data_ptr(), d_idx.data_ptr()
    N.check(det.L.bpmx_pack_trough_floor(det.ctx, ctypes.byref(o), doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         len(nd), 1, ctypes.byref(k), out.data_ptr(), det.stream_handle()),
            "bpmx_pack_trough_floor")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    f_of = np.repeat(np.arange(len(nd)), cnt)
    want = d_floor.cpu().numpy().view(np.uint64)[doff[f_of] + d_idx.cpu().numpy()]
    assert np.array_equal(got[:cap], want[:cap])
    assert (got[cap:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert all(b in got[:cap] for b in special[:3])


# ---- 6. end to end ---------------------------------------------------------------------- #
E2E = [dict(seed=21, secs=14, fs=44100), dict(seed=22, secs=12, fs=44100, channels=2),
       dict(seed=23, secs=20, fs=44100, transform="clicks")]
E2E_HINTS = [None, 70.0, None]
SUFFIXES = ("_bpm_plot.csv", "_Analysis_Summary.md", "_Debug_Log.md", "_Analysis_Settings.json")


@pytest.mark.parametrize("mode", ["reference", "native"])
def test_reports_equal_analyze_wav_file(tmp_path, mode):
    from scipy.io import wavfile
    from bpm_analysis_amd import dropin as D
    from bpm_analysis_amd import plot as PL
    from tests.golden import inputs as I
    src, new, old = tmp_path / "src", tmp_path / "new", tmp_path / "old"
    for p in (src, new, old):
        p.mkdir()
    paths = []
    for k, spec in enumerate(E2E):
        pcm, fs = I.make_input(spec)
        assert pcm.dtype == np.int16
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
    params = dict(C.PARAMS, save_filtered_wav=True)
    got = D.analyze_wav_files_to_reports(paths, params, str(new), start_bpm_hints=E2E_HINTS, mode=mode)
    assert all("error" not in r and r["final_metrics"] is not None for r in got)
    wavs_new = [open(f"{os.path.splitext(p)[0]}_filtered_debug.wav", "rb").read() for p in paths]
    real_plot, PL.write_plot = PL.write_plot, lambda *a, **k: None        # the plot is not part of the comparison
    try:
        for p, h in zip(paths, E2E_HINTS):
            B.analyze_wav_file(p, params, h, p, str(old), mode=mode)
    finally:
        PL.write_plot = real_plot
    for k, p in enumerate(paths):
        base = os.path.basename(os.path.splitext(p)[0])
        for sfx in SUFFIXES:
            a, b = (new / (base + sfx)).read_text(encoding="utf-8"), (old / (base + sfx)).read_text(encoding="utf-8")
            if sfx.endswith(".md"):
                a, b = TB._drop_stamp(a), TB._drop_stamp(b)
            assert a == b, (base, sfx)
        w = (new / f"{base}_filtered_debug.wav").read_bytes()
        assert w == (old / f"{base}_filtered_debug.wav").read_bytes() == wavs_new[k], base
        assert wavs_new[k] == open(f"{os.path.splitext(p)[0]}_filtered_debug.wav", "rb").read(), base
