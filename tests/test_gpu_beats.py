"""bpmx_beats_device (csrc/k_beats.hip) on the MI355X: the beat stages from the
packed peak tables where they lie.  The comparison target is always
``_host.beats_packed`` on the same tables: indices, tags, counts, status and
pass values equal, curves within TB.RTOL (and the tests record whether they
were bit-identical)."""
import ctypes

import numpy as np
import pytest

from bpm_analysis_amd import _host as H
from bpm_analysis_amd import _native as N
from tests import beats_cases as C

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 4, 5, 6, 9, 10, 11, 40, 0, 0, 300, 605, 64, 65, 63, 128, 2, 17, 0, 250, 0]
I32_S, F64_S, I8_S = -7777, -12345.5, 99      # sentinels


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


def _upload(det, tables, cap=None, flags=None):
    """A Packed on the device holding these tables back to back."""
    import torch
    from bpm_analysis_amd.engine import Packed
    cnt = [len(t["idx"]) for t in tables]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    tot = int(off[-1])
    cap = tot if cap is None else cap
    dev = det.device

    def cat(k, dt):
        """The table's first `cap` entries (at least one element, so the tensor has storage)."""
        a = np.concatenate([t[k] for t in tables]).astype(dt)[:cap]
        return torch.from_numpy(a if len(a) else np.zeros(1, dt)).to(dev)

    F = len(tables)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    return Packed(det=det, sr=tables[0]["sr"], doff=np.zeros(F + 1, np.int64), cap_peaks=cap, cap_troughs=0,
                  safe_peaks=tot, safe_troughs=0, pk_off=torch.from_numpy(off).to(dev), tr_off=z,
                  pk_idx=cat("idx", np.int32), pk_env=cat("env", np.float64), pk_floor=cat("flo", np.float64),
                  tr_idx=None, tr_env=None, y16=None, y_max=None,
                  flags=None if flags is None else torch.from_numpy(np.asarray(flags, np.int32)).to(dev))


def _run(det, pk, params, hint):
    """beats_device with every output filled with sentinels first -> host arrays."""
    import torch
    from bpm_analysis_amd.engine import Beats
    F, cap, dev = pk.n_files, max(int(pk.cap_peaks), 1), det.device
    # a few elements beyond the capacity stay in the tensors, to catch a write past it
    full = lambda n, v, dt: torch.full((n + 8,), v, dtype=dt, device=dev)  # noqa: E731
    b = Beats(det=det, packed=pk, final_idx=full(cap, I32_S, torch.int32), n_final=full(F, I32_S, torch.int32),
              bpm_t=full(cap, F64_S, torch.float64), bpm=full(cap, F64_S, torch.float64),
              n_bpm=full(F, I32_S, torch.int32), pass_=full(3 * F, F64_S, torch.float64),
              tags=full(cap, I8_S, torch.int8), status=full(F, I32_S, torch.int32))
    bp = H.beat_params(params)
    k = N.PackedOut()
    k.cap_peaks = pk.cap_peaks
    k.pk_off, k.pk_idx = pk.pk_off.data_ptr(), pk.pk_idx.data_ptr()
    k.pk_env, k.pk_floor = pk.pk_env.data_ptr(), pk.pk_floor.data_ptr()
    o = N.BeatsOut()
    o.final_idx, o.n_final, o.bpm_t, o.bpm = (t.data_ptr() for t in (b.final_idx, b.n_final, b.bpm_t, b.bpm))
    o.n_bpm, o.pass_, o.tags, o.status = (t.data_ptr() for t in (b.n_bpm, b.pass_, b.tags, b.status))
    N.check(det.L.bpmx_beats_device(det.ctx, F, int(pk.sr), ctypes.byref(bp),
                                    float("nan") if hint is None else float(hint), ctypes.byref(k),
                                    None if pk.flags is None else pk.flags.data_ptr(), ctypes.byref(o),
                                    det.stream_handle()), "bpmx_beats_device")
    torch.cuda.synchronize()
    return {f: getattr(b, f).cpu().numpy() for f in ("final_idx", "n_final", "bpm_t", "bpm", "n_bpm", "pass_",
                                                      "tags", "status")}


def _check_batch(raw, tables, off, cap=None, skipped=()):
    """Every file against the host library, and every element no file owns
    against its sentinel.  Returns whether all curves were bit-identical."""
    F = len(tables)
    cap = int(off[-1]) if cap is None else cap
    used = {k: np.zeros(len(raw[k]), bool) for k in ("final_idx", "bpm_t", "bpm", "tags")}
    bits = True
    for f, t in enumerate(tables):
        a, n = int(off[f]), len(t["idx"])
        st, nf, nb = int(raw["status"][f]), int(raw["n_final"][f]), int(raw["n_bpm"][f])
        if f in skipped or a + n > cap:
            assert st == (N.BEATS_SKIPPED if f in skipped else N.BEATS_OVERFLOW), f
            assert nf == 0 and nb == 0 and np.isnan(raw["pass_"][3 * f:3 * f + 3]).all(), f
            continue
        assert 0 <= nf <= n and 0 <= nb <= n, f
        got = dict(status=st, final_peaks=raw["final_idx"][a:a + nf].astype(np.int64), bpm_times=raw["bpm_t"][a:a + nb],
                   bpm=raw["bpm"][a:a + nb], tags=raw["tags"][a:a + n], **{"pass": raw["pass_"][3 * f:3 * f + 3]})
        bits &= C.assert_same(got, t, f"file {f} (n={n})", curves="rtol")
        used["final_idx"][a:a + nf] = True
        used["bpm_t"][a:a + nb] = used["bpm"][a:a + nb] = True
        used["tags"][a:a + n] = True
    for k, s in (("final_idx", I32_S), ("bpm_t", F64_S), ("bpm", F64_S), ("tags", I8_S)):
        assert (raw[k][~used[k]] == s).all(), f"{k}: a write outside the files' counts"
    for k, n in (("n_final", F), ("n_bpm", F), ("status", F), ("pass_", 3 * F)):
        assert (raw[k][n:] == (F64_S if k == "pass_" else I32_S)).all(), k
    return bits


def _crafted():
    return [C.table(*C.craft(n, 50 + f)) for f, n in enumerate(COUNTS)]


def _offsets(tables):
    return np.concatenate([[0], np.cumsum([len(t["idx"]) for t in tables])]).astype(np.int64)


@pytest.mark.parametrize("hint", C.HINTS)
def test_crafted_batch(det, hint, record_property):
    tables = [dict(t, hint=hint) for t in _crafted()]
    raw = _run(det, _upload(det, tables), C.PARAMS, hint)
    bits = _check_batch(raw, tables, _offsets(tables))
    record_property("curves_bit_identical", bits)
    print("curves bit-identical:", bits)


def test_single_file(det):
    t = C.table(*C.craft(300, 62))
    raw = _run(det, _upload(det, [t]), C.PARAMS, None)
    _check_batch(raw, [t], _offsets([t]))


def test_global_workspace_path_gives_the_same(det):
    """The LDS budget forced down (OPT_BEATS_GLOBAL): every file works in global memory."""
    tables = _crafted()
    pk = _upload(det, tables)
    a = _run(det, pk, C.PARAMS, None)
    det.set_options(N.OPT_BEATS_GLOBAL)
    try:
        b = _run(det, pk, C.PARAMS, None)
    finally:
        det.set_options(0)
    _check_batch(b, tables, _offsets(tables))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_long_table_takes_the_global_path(det, record_property):
    t = C.long_table()
    assert len(t["idx"]) > 688                       # beyond the LDS budget (bpmx_plan.h)
    assert C.refinement_fires(t)[0]                   # the gap fill fires: n_fix > 0
    raw = _run(det, _upload(det, [t]), C.PARAMS, None)
    bits = _check_batch(raw, [t], _offsets([t]))
    record_property("curves_bit_identical", bits)
    print("curves bit-identical:", bits)


def test_capacity_smaller_than_the_total(det):
    tables = _crafted()
    off = _offsets(tables)
    cap = int(off[14]) + 20                           # file 14 (64 peaks) straddles it
    assert off[14] < cap < off[15]
    raw = _run(det, _upload(det, tables, cap=cap), C.PARAMS, None)
    _check_batch(raw, tables, off, cap=cap)
    st = raw["status"][:len(tables)]
    assert (st[14:] == N.BEATS_OVERFLOW).all() and (st[:14] != N.BEATS_OVERFLOW).all()


def test_flagged_file_is_skipped(det):
    tables = _crafted()
    flags = np.zeros(len(tables), np.int32)
    flags[12] = N.F_TOO_SHORT
    flags[9] = N.F_STATIC_FLOOR                       # an informative bit skips nothing
    raw = _run(det, _upload(det, tables, flags=flags), C.PARAMS, None)
    _check_batch(raw, tables, _offsets(tables), skipped={12})
    assert raw["status"][12] == N.BEATS_SKIPPED


def test_golden_cases_as_one_batch(det):
    """The reference's own expected results; each case has its own parameters and
    hint, so cases that share them share a launch."""
    gold = C.golden_tables()
    groups = {}
    for name, g, t in gold:
        key = (bytes(H.beat_params(t["params"])), t["hint"], t["sr"])
        groups.setdefault(key, []).append((name, g, t))
    for members in groups.values():
        tables = [t for _, _, t in members]
        off = _offsets(tables)
        raw = _run(det, _upload(det, tables), tables[0]["params"], tables[0]["hint"])
        print("curves bit-identical:", _check_batch(raw, tables, off))
        for f, (name, g, t) in enumerate(members):
            a, n = int(off[f]), len(t["idx"])
            nf, nb = int(raw["n_final"][f]), int(raw["n_bpm"][f])
            got = dict(status=int(raw["status"][f]), final_peaks=raw["final_idx"][a:a + nf].astype(np.int64),
                       bpm_times=raw["bpm_t"][a:a + nb], bpm=raw["bpm"][a:a + nb], tags=raw["tags"][a:a + n],
                       **{"pass": raw["pass_"][3 * f:3 * f + 3]})
            C.assert_golden(got, g, name)


# ---- through the pipeline ---------------------------------------------------- #
FRAMES = [44100 * 9, 44100 * 14 + 3, 146 * 15, 44100 * 11]


@pytest.fixture(scope="module")
def recordings():
    from oracle import oracle as O
    return [O.synth(60 + i, n, 44100, 1) for i, n in enumerate(FRAMES)]


def _same_dict(a, b, what):
    assert sorted(a) == sorted(b), what
    for k, v in a.items():
        if k == "error":
            assert type(v) is type(b[k]) and v.args == b[k].args, what
        elif isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype, (what, k)
            if v.dtype.kind == "f":
                np.testing.assert_allclose(v, b[k], rtol=C.TB.RTOL, atol=0, equal_nan=True)
            else:
                assert np.array_equal(v, b[k]), (what, k)
        else:
            assert v == b[k], (what, k)


@pytest.mark.parametrize("mode", ["native", "reference"])
def test_run_host_beats_equals_packed_then_host_library(det, recordings, mode):
    got = det.run_host_beats(recordings, 44100, C.PARAMS, mode=mode)
    packed = det.run_host_packed(recordings, 44100, C.PARAMS, mode=mode, resolve_ties=True)
    assert len(got) == len(packed) == len(recordings)
    for f, (g, p) in enumerate(zip(got, packed)):
        assert g["flags"] == p["flags"], f
        if p["flags"] & N.F_TOO_SHORT:
            assert g.get("skipped") is True and len(g["raw_peaks"]) == 0, f
            continue
        want = H.beats_packed(p["peaks"], p["env_pk"], p["floor_pk"], p["n_env"], p["sr"], C.PARAMS, None)
        want = dict(want, raw_peaks=p["peaks"], flags=p["flags"])
        _same_dict(g, want, f"file {f}")
    assert got[2].get("skipped") is True and len(got[0]["final_peaks"]) > 2


def test_run_sharded_device_equals_native(det, recordings):
    from bpm_analysis_amd.shard import run_sharded
    kw = dict(fs=44100, mode="native", detector=det, host_threads=2, chunk_frames=44100 * 20)
    a = run_sharded(recordings, C.PARAMS, beats="native", **kw)
    b = run_sharded(recordings, C.PARAMS, beats="device", **kw)
    assert len(a) == len(b) == len(recordings)
    for f, (x, y) in enumerate(zip(a, b)):
        _same_dict(y, x, f"file {f}")
    assert isinstance(b[2]["error"], ValueError) and "padlen" in str(b[2]["error"])
    assert len(b[0]["final_peaks"]) > 2 and len(b[0]["bpm"]) > 2
