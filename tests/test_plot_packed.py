"""The analysis figure from packed tables (plot.build_figure_packed), no GPU.

The device route holds a recording as bpmx_pack's tables (env and floor at the
raw peaks and the troughs) plus the two plot series ``env[::kf]`` and
``floor[::kf]`` (bpmx_pack_plot).  Here those are cut from the golden inputs
with numpy; the figure built from them must be the reference's: the existing
beat goldens carry plot_downsample_factor 1, tests/golden/beats/plot/*.npz
(make_plot_goldens.py) the reference's figures at 5, at a factor beyond the
envelope's length and at one equal to it.  Figures are compared as plotly JSON,
character for character (through the golden's sha256).
"""
from __future__ import annotations

import functools
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import beats as B
from bpm_analysis_amd import engine as E
from bpm_analysis_amd import plot as PL
from tests import test_beats as TB

HERE = os.path.dirname(os.path.abspath(__file__))
PLOT_GOLD = os.path.join(HERE, "golden", "beats", "plot")
PLOT_CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(PLOT_GOLD, "*.npz")))


def ref_kf(n, k):
    """The reference's stride for n envelope samples (bpm_analysis.py:518-519)."""
    return k if (k > 1 and n >= k) else 1


@pytest.mark.parametrize("factor", [-3, 0, 1, 2, 5, 7, 18124, 18125])
@pytest.mark.parametrize("nd", [0, 1, 4, 5, 6, 16, 18124])
def test_plot_length(nd, factor):
    assert N.load().bpmx_plot_length(nd, factor) == len(np.empty(nd)[::ref_kf(nd, factor)])


def test_device_factor():
    """What is not an integer above 1 keeps whole series; an integer is clamped to int32."""
    for given, want in [(5, 5), (1, 1), (0, 1), (-3, 1), (2 ** 40, 2 ** 31 - 1), (2.5, 1), (5.0, 1), ("5", 1),
                        (None, 1), (True, 1), (np.int64(7), 7), (np.int32(2), 2)]:
        assert E.plot_device_factor(given) == want, given


@functools.lru_cache(maxsize=None)
def analysed(source, hinted=False):
    """(golden, params, inputs, analyze_recording's result) of a beat golden, computed once."""
    g, params, hint, inp = TB.load_case(source + ("_hint" if hinted else ""))
    if "fig_sha256" not in g:
        return g, params, inp, None
    res = B.analyze_recording(inp["env"], inp["sr"], inp["floor"], inp["troughs"], inp["peaks"], params, hint)
    return g, params, inp, res


def packed(inp, res, kf):
    """The per-file dict of Detector.run_host_reports(plot=True), cut with
    numpy; no whole array and nothing derived from one is left in it."""
    env, floor = np.asarray(inp["env"], np.float64), np.asarray(inp["floor"], np.float64)
    pk, tr = np.asarray(res["all_raw_peaks"], np.int64), np.asarray(inp["troughs"], np.int64)
    data = {k: v for k, v in res["analysis_data"].items() if k not in ("trough_indices", "dynamic_noise_floor_series")}
    return dict(sr=inp["sr"], n_env=len(env), peaks=pk, env_pk=env[pk], floor_pk=floor[pk], troughs=tr,
                env_tr=env[tr], floor_tr=floor[tr], env_plot=env[::kf].copy(), floor_plot=floor[::kf].copy(),
                plot_factor=kf, analysis_data=data, final_metrics=res["final_metrics"])


def sha(fig):
    return hashlib.sha256(fig.to_json().encode()).hexdigest()


@pytest.mark.parametrize("name", TB.CASES)
def test_packed_figure_matches_reference_k1(name):
    hinted = name.endswith("_hint")
    g, params, inp, res = analysed(name[:-5] if hinted else name, hinted)
    if res is None:
        assert "fig_sha256" not in g        # the reference draws no figure: nothing to rebuild
        return
    assert params["plot_downsample_factor"] == 1
    fig = PL.build_figure_packed(name + ".wav", params, packed(inp, res, 1))
    assert sha(fig) == str(g["fig_sha256"])


@pytest.mark.parametrize("name", PLOT_CASES)
def test_packed_figure_matches_reference_other_factors(name):
    g = np.load(os.path.join(PLOT_GOLD, name + ".npz"))
    _, params, inp, res = analysed(str(g["source"]))
    k = int(g["factor"])
    params = dict(params, plot_downsample_factor=k)
    assert json.loads(str(g["params"]))["plot_downsample_factor"] == k
    n = len(inp["env"])
    kf = ref_kf(n, k)
    assert N.load().bpmx_plot_length(n, E.plot_device_factor(k)) == len(inp["env"][::kf])
    js = PL.build_figure_packed(name + ".wav", params, packed(inp, res, kf)).to_json()
    if "fig_json" in g:
        want, got = json.loads(str(g["fig_json"])), json.loads(js)
        assert len(got["data"]) == len(want["data"])
        for i, (a, b) in enumerate(zip(got["data"], want["data"])):
            assert a == b, f"trace {i} ({b.get('name')})"
        assert got["layout"] == want["layout"]
    assert hashlib.sha256(js.encode()).hexdigest() == str(g["fig_sha256"])


def test_plot_goldens_cover_the_rule():
    """A strided case, a factor beyond the length and one equal to it."""
    kinds = set()
    for name in PLOT_CASES:
        g = np.load(os.path.join(PLOT_GOLD, name + ".npz"))
        n, k = int(g["n_env"]), int(g["factor"])
        kinds.add("beyond" if k > n else "equal" if k == n else "strided")
    assert kinds == {"beyond", "equal", "strided"}


@pytest.mark.parametrize("factor", [2, 5, 64])
@pytest.mark.parametrize("source", ["ref_44k_60s_mono", "ref_44k_40s_clicks", "vulpine"])
def test_packed_equals_dense(source, factor):
    _, params, inp, res = analysed(source)
    params = dict(params, plot_downsample_factor=factor)
    dense = PL.build_figure(source + ".wav", params, inp["sr"], np.asarray(inp["env"], np.float64),
                            res["all_raw_peaks"], res["analysis_data"], res["final_metrics"])
    got = PL.build_figure_packed(source + ".wav", params, packed(inp, res, ref_kf(len(inp["env"]), factor)))
    assert got.to_json() == dense.to_json()


def test_without_floor_series():
    """``floor_plot`` None (pack_plot(want_floor=False)): the figure of a recording without a floor series."""
    _, params, inp, res = analysed("ref_44k_12s_f32")
    params = dict(params, plot_downsample_factor=5)
    data = dict(res["analysis_data"], dynamic_noise_floor_series=None)
    dense = PL.build_figure("a.wav", params, inp["sr"], np.asarray(inp["env"], np.float64), res["all_raw_peaks"],
                            data, res["final_metrics"])
    r = packed(inp, res, 5)
    r["floor_plot"] = None
    assert PL.build_figure_packed("a.wav", params, r).to_json() == dense.to_json()


@pytest.mark.parametrize("factor", ["5", None, 2.5, 5.0, 0.5, 1.0, 1e9, True])
def test_factor_that_is_no_int_behaves_as_dense(factor):
    """The packed route validates the factor no more than the reference does:
    the same exception from the same statement, or the same figure."""
    _, params, inp, res = analysed("ref_44k_12s_f32")
    params = dict(params, plot_downsample_factor=factor)
    r = packed(inp, res, ref_kf(len(inp["env"]), E.plot_device_factor(factor)))

    def outcome(fn):
        try:
            return "figure", fn().to_json()
        except Exception as exc:                       # noqa: BLE001 - the comparison is the point
            tb = exc.__traceback__
            while tb.tb_next is not None and tb.tb_frame.f_code.co_name != "build_figure":
                tb = tb.tb_next
            return type(exc), str(exc), tb.tb_frame.f_code.co_name, tb.tb_lineno

    dense = outcome(lambda: PL.build_figure("a.wav", params, inp["sr"], np.asarray(inp["env"], np.float64),
                                            res["all_raw_peaks"], res["analysis_data"], res["final_metrics"]))
    assert outcome(lambda: PL.build_figure_packed("a.wav", params, r)) == dense


def test_write_plot_packed(tmp_path):
    _, params, inp, res = analysed("ref_44k_12s_f32")
    params = dict(params, plot_downsample_factor=5)
    fig = PL.write_plot_packed(os.path.join(str(tmp_path), "rec.wav"), str(tmp_path), params, packed(inp, res, 5))
    assert fig.to_json() == PL.build_figure_packed("rec.wav", params, packed(inp, res, 5)).to_json()
    assert (tmp_path / "rec_bpm_plot.html").stat().st_size > 0
