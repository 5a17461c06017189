"""The rectified mode's constants in include/bpmx.h against the Python layer,
and the design helper the mode uses (no GPU)."""
import os
import re

from bpm_analysis_amd import DEFAULT_PARAMS
from bpm_analysis_amd import _native as N
from bpm_analysis_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "bpmx.h")) as f:
        return f.read()


def _enum(name):
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, _header())
    assert m, name
    return int(m.group(1))


def test_header_constants_match_native():
    assert _enum("BPMX_MODE_RECTIFIED") == N.MODE_RECTIFIED == 2
    assert _enum("BPMX_OPT_RECT_SEQ") == N.OPT_RECT_SEQ == 65536
    assert (_enum("BPMX_MODE_REFERENCE"), _enum("BPMX_MODE_NATIVE")) == (N.MODE_REFERENCE, N.MODE_NATIVE)
    # a new bit of its own
    others = [int(v) for k, v in re.findall(r"\b(BPMX_OPT_\w+)\s*=\s*(\d+)", _header()) if k != "BPMX_OPT_RECT_SEQ"]
    assert others and all(v & N.OPT_RECT_SEQ == 0 for v in others)


def test_abi_version_unchanged_and_addition_noted():
    h = _header()
    assert re.search(r"#define BPMX_ABI_VERSION 4\b", h)
    note = h[:h.index("#define BPMX_ABI_VERSION")][-400:]
    assert "BPMX_MODE_RECTIFIED" in note and "BPMX_OPT_RECT_SEQ" in note


def test_modes():
    assert engine.MODES == {"reference": N.MODE_REFERENCE, "native": N.MODE_NATIVE, "rectified": N.MODE_RECTIFIED}


def test_design_helper_takes_the_rate_as_it_is(caplog):
    """fs 302 with downsample_factor 300 makes design() clamp and warn; the
    rectified mode neither decimates nor designs a filter."""
    params = dict(DEFAULT_PARAMS, downsample_factor=300)
    with caplog.at_level("WARNING"):
        d = engine.mode_design(302, params, "rectified", log=True)
    assert (d.ds, d.sr, d.fs, d.env_window, d.warnings) == (1, 302, 302, 30, ())
    assert not caplog.records
    assert d.distance == int(params["min_peak_distance_sec"] * 302)
    assert d.noise_window == int(params["noise_window_sec"] * 302)
    # the other modes still go through design(), which clamps and warns here
    ref = engine.mode_design(302, params, "reference")
    assert ref == engine.design(302, params, log=False) and len(ref.warnings) == 2 and any(ref.b)
