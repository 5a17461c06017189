"""bpmx_pack_plot on the GPU and the plot at the end of the device route.

1. The copy, bit for bit: ragged batches whose env and floor the test fills
   itself (random f64 with NaN payloads, -0.0, infinities and denormals), at
   factors on every side of the keep rule; outputs pre-filled with 0xFF and
   compared as uint64 with numpy's slices, 0xFF intact past the total.
2. End to end: ``dropin.analyze_wav_files_to_reports(plot=True)`` returns the
   figure the full-download route (``beats.analyze_wav_file``) draws for the
   same files, as plotly JSON, in both modes at factors 1 and 5.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from bpm_analysis_amd import engine as E
from tests import beats_cases as C
from tests import test_beats as TB
from tests import test_gpu_trace as GT

pytestmark = pytest.mark.gpu

PAD = 8                                                # elements kept beyond every capacity
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
# every length of the issue's list, ordered so that slices start at odd offsets
# and the 5000-sample file is followed by files a factor near 5000 leaves whole
RAGGED = [65, 5000, 17, 1024, 63, 16, 1025, 64, 1023]
FACTORS = [1, 2, 5, 7, 64, 4999, 5000, 5001]
SPECIAL = np.array([0x7FF8000000ABCDEF, 0xFFF80000DEADBEEF, 0x7FF0000000000001, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF], np.uint64)


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    d = Detector(0)
    yield d
    d.close()


def _series(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    pos = rng.choice(n, max(n // 11, min(n, len(SPECIAL))), replace=False)
    a.view(np.uint64)[pos] = SPECIAL[np.arange(len(pos)) % len(SPECIAL)]
    return a


@pytest.fixture(scope="module")
def inputs(det):
    """nds -> (doff, env, floor on the host, env, floor on the device), made once per batch shape."""
    import torch
    made = {}

    def get(nds):
        key = tuple(nds)
        if key not in made:
            doff = np.concatenate([[0], np.cumsum(nds)]).astype(np.int64)
            env, floor = _series(int(doff[-1]), 1), _series(int(doff[-1]), 2)
            made[key] = (doff, env, floor, torch.from_numpy(env).to(det.device), torch.from_numpy(floor).to(det.device))
        return made[key]

    return get


def ref_kf(n, k):
    return k if (k > 1 and n >= k) else 1


def _want(a, doff, factor):
    parts = [a[doff[f]:doff[f + 1]][::ref_kf(int(doff[f + 1] - doff[f]), factor)] for f in range(len(doff) - 1)]
    return np.concatenate(parts).view(np.uint64)


def _pack(det, inp, factor, want_floor=True, cap=None, shift=0):
    """bpmx_pack_plot into 0xFF-filled buffers (written from element `shift` on)
    -> (rc, env out, floor out as uint64, the total by the rule)."""
    import torch
    doff, env, floor, d_env, d_floor = inp
    tot = int(sum(N.load().bpmx_plot_length(int(n), factor) for n in np.diff(doff)))
    cap = tot if cap is None else cap
    oe = torch.full((shift + tot + PAD,), -1, dtype=torch.int64, device=det.device)
    of = torch.full((shift + tot + PAD,), -1, dtype=torch.int64, device=det.device)
    o = N.Out()
    o.env, o.floor = d_env.data_ptr(), d_floor.data_ptr()
    rc = det.L.bpmx_pack_plot(det.ctx, len(doff) - 1, doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, factor,
                              ctypes.byref(o), oe.data_ptr() + 8 * shift,
                              of.data_ptr() + 8 * shift if want_floor else None, cap, det.stream_handle())
    torch.cuda.synchronize()
    return rc, oe.cpu().numpy().view(np.uint64), of.cpu().numpy().view(np.uint64), tot


def _check_copy(det, inp, factor, shift=0):
    doff, env, floor = inp[:3]
    rc, ge, gf, tot = _pack(det, inp, factor, shift=shift)
    assert rc == N.OK, N.load().bpmx_last_error()
    we, wf = _want(env, doff, factor), _want(floor, doff, factor)
    assert len(we) == tot
    for got, want in ((ge, we), (gf, wf)):
        assert (got[:shift] == FF).all()
        assert np.array_equal(got[shift:shift + tot], want)
        assert (got[shift + tot:] == FF).all()


@pytest.mark.parametrize("factor", FACTORS)
def test_ragged_copy(det, inputs, factor):
    inp = inputs(RAGGED)
    assert all(b in inp[1].view(np.uint64) for b in SPECIAL)
    _check_copy(det, inp, factor)


@pytest.mark.parametrize("factor", FACTORS)
def test_one_long_file(det, inputs, factor):
    _check_copy(det, inputs([576000]), factor)


@pytest.mark.parametrize("factor", [1, 5])
def test_single_short_file(det, inputs, factor):
    _check_copy(det, inputs([1025]), factor)


@pytest.mark.parametrize("factor", [1, 5])
def test_output_off_the_16_byte_phase_of_the_input(det, inputs, factor):
    _check_copy(det, inputs(RAGGED), factor, shift=1)


def test_without_floor(det, inputs):
    inp = inputs(RAGGED)
    rc, ge, gf, tot = _pack(det, inp, 5, want_floor=False)
    assert rc == N.OK
    assert np.array_equal(ge[:tot], _want(inp[1], inp[0], 5)) and (ge[tot:] == FF).all()
    assert (gf == FF).all()


@pytest.mark.parametrize("factor", [1, 5])
def test_capacity_one_short_writes_nothing(det, inputs, factor):
    inp = inputs(RAGGED)
    tot = int(sum(N.load().bpmx_plot_length(int(n), factor) for n in RAGGED))
    rc, ge, gf, _ = _pack(det, inp, factor, cap=tot - 1)
    assert rc == N.E_ARG and b"cap" in N.load().bpmx_last_error()
    assert (ge == FF).all() and (gf == FF).all()


def _result(inp):
    doff, _, _, d_env, d_floor = inp
    return E.Result(sr=302, ds=1, frame_offsets=doff, doff=doff, env=d_env, floor=d_floor, y=None, troughs=None,
                    peaks=None, n_troughs=None, n_peaks=None, n_raw_troughs=None, flags=None)


@pytest.mark.parametrize("factor", [1, 5, 5000])
def test_engine_series(det, inputs, factor):
    """Detector.pack_plot + PlotSeries.to_host: per file numpy's slices and the
    kf used; at factor 1 the Result's own tensors, nothing launched."""
    import torch
    inp = inputs(RAGGED)
    doff, env, floor = inp[:3]
    with det.lock, torch.cuda.stream(det.host_stream()):
        ps = det.pack_plot(_result(inp), factor)
        got = ps.to_host()
        nofloor = det.pack_plot(_result(inp), factor, want_floor=False).to_host()
    assert (ps.env is inp[3]) == (factor == 1)
    for f, r in enumerate(got):
        kf = ref_kf(RAGGED[f], factor)
        assert r["plot_factor"] == kf
        assert np.array_equal(r["env_plot"].view(np.uint64), env[doff[f]:doff[f + 1]][::kf].view(np.uint64))
        assert np.array_equal(r["floor_plot"].view(np.uint64), floor[doff[f]:doff[f + 1]][::kf].view(np.uint64))
        assert nofloor[f]["floor_plot"] is None
        assert np.array_equal(nofloor[f]["env_plot"].view(np.uint64), r["env_plot"].view(np.uint64))


def test_engine_capacity(det, inputs):
    import torch
    inp = inputs(RAGGED)
    tot = int(sum(N.load().bpmx_plot_length(int(n), 1) for n in RAGGED))
    small = torch.full((tot - 1,), -1, dtype=torch.int64, device=det.device).view(torch.float64)
    with pytest.raises(N.BpmxArgError):
        det.pack_plot(_result(inp), 1, want_floor=False, out=(small, None))
    torch.cuda.synchronize()
    assert (small.view(torch.int64) == -1).all()


# ---- end to end ------------------------------------------------------------------------ #
def _wavs(src):
    from scipy.io import wavfile
    from tests.golden import inputs as I
    paths = []
    for k, spec in enumerate(GT.E2E):
        pcm, fs = I.make_input(spec)
        paths.append(str(src / f"rec{k}.wav"))
        wavfile.write(paths[-1], fs, pcm)
    return paths


@pytest.mark.parametrize("factor", [1, 5])
@pytest.mark.parametrize("mode", ["reference", "native"])
def test_figures_equal_the_full_download_route(tmp_path, monkeypatch, mode, factor):
    from bpm_analysis_amd import dropin as D
    from bpm_analysis_amd import plot as PL
    src, new, old = tmp_path / "src", tmp_path / "new", tmp_path / "old"
    for p in (src, new, old):
        p.mkdir()
    paths = _wavs(src)
    params = dict(C.PARAMS, plot_downsample_factor=factor)
    got = D.analyze_wav_files_to_reports(paths, params, str(new), start_bpm_hints=GT.E2E_HINTS, mode=mode, plot=True)
    assert all("error" not in r and r["final_metrics"] is not None for r in got)
    dense, real = [], PL.write_plot
    monkeypatch.setattr(PL, "write_plot", lambda *a, **k: dense.append(real(*a, **k)))
    for p, h in zip(paths, GT.E2E_HINTS):
        B.analyze_wav_file(p, params, h, p, str(old), mode=mode)
    assert len(dense) == len(paths)
    for p, r, fig in zip(paths, got, dense):
        base = os.path.basename(os.path.splitext(p)[0])
        assert r["plot_factor"] == factor
        assert r["figure"].to_json() == fig.to_json(), base
        assert (new / f"{base}_bpm_plot.html").stat().st_size > 0
        assert (old / f"{base}_bpm_plot.html").stat().st_size > 0


def test_plot_false_is_unchanged(tmp_path):
    """Without ``plot`` no figure, no series and no HTML; with it the other files are the same."""
    from bpm_analysis_amd import dropin as D
    src, off, on = tmp_path / "src", tmp_path / "off", tmp_path / "on"
    for p in (src, off, on):
        p.mkdir()
    paths = _wavs(src)
    params = dict(C.PARAMS, plot_downsample_factor=5)
    a = D.analyze_wav_files_to_reports(paths, params, str(off), start_bpm_hints=GT.E2E_HINTS)
    b = D.analyze_wav_files_to_reports(paths, params, str(on), start_bpm_hints=GT.E2E_HINTS, plot=True)
    for ra, rb in zip(a, b):
        assert set(rb) - set(ra) == {"env_plot", "floor_plot", "plot_factor", "figure"} and set(ra) <= set(rb)
        for k in ("peaks", "env_pk", "floor_pk", "troughs", "env_tr", "floor_tr", "final_peaks"):
            assert np.array_equal(ra[k], rb[k]), k
    names = sorted(os.listdir(off))
    assert names == sorted(f"rec{k}{s}" for k in range(len(paths)) for s in GT.SUFFIXES)
    assert sorted(os.listdir(on)) == sorted(names + [f"rec{k}_bpm_plot.html" for k in range(len(paths))])
    for n in names:
        x, y = (off / n).read_text(encoding="utf-8"), (on / n).read_text(encoding="utf-8")
        if n.endswith(".md"):
            x, y = TB._drop_stamp(x), TB._drop_stamp(y)
        assert x == y, n
