"""Fixtures for the analysis of a person's corrected marks, made by the
reference's own functions.

    python tests/golden/make_marks_goldens.py /path/to/reference

Takes the label tables of a handful of beat goldens (tests/golden/labels/*.npz:
``time``, ``type``) and corrects them the way a person does in the labeler, with
a seeded generator: marks moved by some milliseconds, removed, given the other
name, added, and typed twice on one millisecond.  The corrected table goes
through the project's rule (labels.rows_from_marks: rows on the sample grid,
the S1 rows are the final beats); everything behind that rule is the
reference's: ``_calculate_final_metrics`` on the S1 indices (curve, times, HRV
frame, slopes, HRR, inclines and declines, summary), ``ReportGenerator.
save_analysis_summary``'s text, the BPM CSV that ``Plotter.plot_and_save``
writes, and the labeler's ``calculate_s1_s2_diffs`` / ``detect_labeling_groups``
/ ``calculate_group_statistics`` / ``save_labels`` on the re-stated table
(make_label_goldens.run_labeler).  The results are stored as data in
tests/golden/marks/<name>.npz: arrays and text.

No program text of the reference is stored.
"""
import json
import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_label_goldens as ML  # noqa: E402
from bpm_analysis_amd import labels as LB  # noqa: E402

CASES = ("ref_44k_40s_clicks", "nat_44k_60s_mono", "ref_22k_30s_mono", "env_random_rough", "vulpine")
MOVE_MS = (40, 40, 40, 40, 6)      # the long recording keeps its inclines and declines under small moves


def correct(time, typ, seed, move_ms=40):
    """A corrected table from a label table: (time, type), in file order."""
    rng = np.random.default_rng(seed)
    ms = np.rint(np.asarray(time) * 1000.0).astype(np.int64)
    typ = np.asarray(typ).astype(np.int64)
    n = len(ms)
    u = rng.random(n)
    ms = ms + np.where(u < 0.3, rng.integers(-move_ms, move_ms + 1, n), 0)                  # moved
    typ = np.where(rng.random(n) < 0.06, 3 - typ, typ)                        # the other name
    keep = rng.random(n) >= 0.08                                              # removed
    ms, typ = ms[keep], typ[keep]
    k = max(2, n // 15)                                                       # added
    ms = np.concatenate([ms, rng.integers(int(ms.min()), int(ms.max()) + 1500, k)])
    typ = np.concatenate([typ, rng.integers(1, 3, k)])
    d = rng.choice(len(ms), size=max(1, n // 30), replace=False)              # typed twice
    ms, typ = np.concatenate([ms, ms[d]]), np.concatenate([typ, 3 - typ[d]])
    order = rng.permutation(len(ms))                                          # a file need not be in order
    return ms[order] / 1000.0, typ[order]


def _ts(v):
    import pandas as pd
    if isinstance(v, pd.Timestamp):
        return {"ns": int(v.value)}
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return v


def metrics_json(m):
    d = {}
    for k in ("major_inclines", "major_declines"):
        d[k] = [{kk: _ts(vv) for kk, vv in x.items()} for x in m[k]]
    for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
        d[k] = None if m[k] is None else {kk: _ts(vv) for kk, vv in m[k].items()}
    d["hrv_summary"] = {k: float(v) for k, v in m["hrv_summary"].items()}
    return json.dumps(d)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BPMX_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: make_marks_goldens.py /path/to/reference")
    np.seterr(all="ignore")
    logging.getLogger().setLevel(logging.ERROR)
    L, _ = ML._reference(ref)
    import bpm_analysis as R
    import config as RC
    out_dir = os.path.join(HERE, "marks")
    os.makedirs(out_dir, exist_ok=True)
    for c, name in enumerate(CASES):
        lab = np.load(os.path.join(HERE, "labels", name + ".npz"))
        g = np.load(os.path.join(HERE, "beats", name + ".npz"))
        sr = int(g["sr"])
        params = dict(RC.DEFAULT_PARAMS)
        params.update(json.loads(str(g["params"])))
        time, typ = correct(lab["time"], lab["type"], 900 + c, MOVE_MS[c])
        table = LB._table([-1] * len(typ), typ, time, np.full(len(typ), 60.0))
        rows = LB.rows_from_marks(table, sr)
        fin = rows["final"]
        m = R._calculate_final_metrics(fin, sr, params)
        sb, h = m["smoothed_bpm"], m["windowed_hrv_df"]
        out = dict(none=np.bool_(False), sr=np.int64(sr), params=np.str_(json.dumps({k: params[k] for k in RC.DEFAULT_PARAMS})),
                   c_time=time, c_type=typ.astype(np.int8), row_idx=rows["idx"], row_type=rows["type"],
                   record=rows["record"], final_peaks=fin, bpm_times=np.asarray(m["bpm_times"], dtype=float),
                   bpm_v=sb.to_numpy(float), metrics=np.str_(metrics_json(m)))
        for col in ("time", "rmssdc", "sdnn", "bpm"):
            out["hrv_" + col] = h[col].to_numpy(float) if len(h) else np.zeros(0)
        with tempfile.TemporaryDirectory() as td:
            wav = os.path.join(td, name + "_corrected.wav")
            rep = R.ReportGenerator(wav, td)
            rep.save_analysis_summary(m)
            lines = open(os.path.join(td, name + "_corrected_Analysis_Summary.md"), encoding="utf-8").read().split("\n")
            out["summary_md"] = np.str_("\n".join(lines[:1] + lines[2:]))     # without the timestamp line
            # the CSV is written at the end of the figure's method: an envelope of zeros, no decision trace
            env = np.zeros(int(rows["idx"][-1]) + 2)
            R.Plotter(wav, params, sr, td).plot_and_save(env, rows["idx"], {}, m)
            out["csv"] = np.str_(open(os.path.join(td, name + "_corrected_bpm_plot.csv")).read())
        T, B = ML.csv_floats(out["csv"])
        out.update(ML.run_labeler(L, name + "_corrected", rows["idx"], rows["type"], sr, T, B))
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **out)
        print(f"{name}: {len(typ)} marks, record {rows['record'].tolist()}, {len(sb)} curve rows, {len(h)} HRV rows, "
              f"{len(out['pair_dt'])} pairs, {os.path.getsize(os.path.join(out_dir, name + '.npz'))} bytes")


if __name__ == "__main__":
    main()
