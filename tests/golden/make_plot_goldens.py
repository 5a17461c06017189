"""Golden figures at a plot_downsample_factor other than 1, from the REFERENCE.

Runs only in the build container, where ``/root/reference`` is importable (like
make_beat_goldens.py, whose goldens all carry the shipped factor 1).  For a few
hot-path goldens (tests/golden/<source>.npz: env / floor / troughs) it runs the
reference's stages 2-6 of ``analyze_wav_file`` (bpm_analysis.py:1734-1757) with
``plot_downsample_factor`` set, and records the ``Plotter`` figure's plotly
JSON (:429-780; the line traces keep every factor-th sample, :518-524) as data
in ``tests/golden/beats/plot/<source>_k<factor>.npz``: ``fig_sha256`` always,
``fig_json`` when shorter than 600 000 characters.

    python tests/golden/make_plot_goldens.py
"""
from __future__ import annotations

import hashlib
import json
import logging
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "beats", "plot")

sys.path.insert(0, "/root/reference")
import bpm_analysis as R  # noqa: E402
import config as RC  # noqa: E402

# (source golden, factor): two short recordings at 5, a factor beyond the
# envelope's length (the reference then keeps the whole series) and one equal
# to it (a single sample is kept)
CASES = [
    ("ref_44k_12s_f32", 5),
    ("ref_44k_40s_clicks", 5),
    ("env_static_fallback", 1001),
    ("env_draft_fallback", 1100),
]


def run_case(name, env, sr, floor, troughs, params):
    floor_s = pd.Series(floor, index=np.arange(len(floor)))
    start, t_pk, t_end = R._run_preliminary_pass(env, sr, params, floor_s, troughs, None)
    clf = R.PeakClassifier(env, sr, params, start, floor_s, troughs, t_pk, t_end)
    s1, raw, data = clf.classify_peaks()
    final, data = R._refine_and_correct_peaks(s1, raw, data, env, sr, params)
    m = R._calculate_final_metrics(final, sr, params)
    with tempfile.TemporaryDirectory() as td:
        p = R.Plotter(os.path.join(td, name + ".wav"), params, sr, td)
        return p.plot_and_save(env, raw, data, m).to_json()


def main():
    np.seterr(all="ignore")
    logging.getLogger().setLevel(logging.ERROR)
    os.makedirs(OUT, exist_ok=True)
    for source, factor in CASES:
        g = np.load(os.path.join(HERE, source + ".npz"))
        params = dict(RC.DEFAULT_PARAMS)
        params.update(json.loads(str(g["params"])))
        params["plot_downsample_factor"] = factor
        name = f"{source}_k{factor}"
        fig_json = run_case(name, g["env"], int(g["sr"]), g["floor"], g["troughs"], params)
        o = dict(name=name, source=source, factor=factor, n_env=len(g["env"]),
                 params=json.dumps({k: params[k] for k in params if k in RC.DEFAULT_PARAMS}),
                 fig_sha256=hashlib.sha256(fig_json.encode()).hexdigest())
        if len(fig_json) < 600_000:
            o["fig_json"] = fig_json
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **o)
        print(name, len(g["env"]), len(fig_json))


if __name__ == "__main__":
    main()
