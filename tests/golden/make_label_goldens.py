"""Label fixtures made by the reference labeler's own functions.

    python tests/golden/make_label_goldens.py /path/to/reference

Reads the beat goldens (tests/golden/beats/*.npz: ``final_peaks``,
``info_keys`` / ``info_vals``, ``csv``, ``sr``), selects the labels as
bpm_analysis_amd/labels.py defines them (S1: every final beat; S2: every other
raw peak whose final debug string satisfies the reference's ``PeakType.is_s2``)
and runs heartbeat_labeler.py's ``find_nearest_idx``,
``calculate_s1_s2_diffs``, ``detect_labeling_groups``,
``calculate_group_statistics``, ``calculate_avg_delta_t_in_range``,
``save_labels`` and ``load_labels`` on them.  The results are stored as data in
tests/golden/labels/<name>.npz: arrays and the file text, with groups at gaps
1, 3.0 and 5.0.  The CSV rows (T, B) are read with Python's ``float``.

``_random.npz`` holds a few dozen small random cases through the same
functions: ragged S1 / S2 orders, runs of S2 before the first S1, single-S1
groups, steps exactly at the gap threshold.  Each is given as raw peaks at
sr = 1000 with a type per peak and a curve, so the same case runs through
labels.py, the core header and the kernel.

No program text of the reference is stored.
"""
import glob
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
GAPS = (1, 3.0, 5.0)
COLS = ["Time (s)", "Average BPM", "Peak Type"]


def _reference(path):
    sys.path.insert(0, path)
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())                      # the labeler lists processed_files/ on import
    try:
        import bpm_analysis
        import heartbeat_labeler
    finally:
        os.chdir(cwd)
    return heartbeat_labeler, bpm_analysis.PeakType


def run_labeler(L, name, raw, types, sr, T, B):
    """The labeler's functions on the typed raw peaks -> dict of arrays."""
    rows, pos = [], []
    time_axis_at = lambda i: np.float64(i) / sr       # np.arange(n) / sample_rate at i  # noqa: E731
    for i in np.flatnonzero(types).tolist():
        x = float(time_axis_at(int(raw[i])))
        k = L.find_nearest_idx(T, x)
        rows.append({"Time (s)": round(x, 3), "Average BPM": round(float(B[k]), 3),
                     "Peak Type": "S1" if types[i] == 1 else "S2"})
        pos.append(i)
    df = pd.DataFrame(rows, columns=COLS)
    if len(df):
        assert df["Time (s)"].is_monotonic_increasing and df["Time (s)"].is_unique, name
        df = df.sort_values("Time (s)").reset_index(drop=True)
    out = {"pos": np.asarray(pos, np.int64), "type": np.asarray([1 if t == "S1" else 2 for t in df["Peak Type"]], np.int8),
           "time": df["Time (s)"].to_numpy(np.float64), "bpm": df["Average BPM"].to_numpy(np.float64)}
    pairs = L.calculate_s1_s2_diffs(df)
    pa = np.asarray(pairs, np.float64).reshape(-1, 4)
    out.update(pair_s1_time=pa[:, 0].copy(), pair_s2_time=pa[:, 1].copy(), pair_dt=pa[:, 2].copy(),
               pair_s1_bpm=pa[:, 3].copy())
    for gap in GAPS:
        st = L.calculate_group_statistics(df, L.detect_labeling_groups(df, gap)) if len(df) else []
        tag = f"g{gap}_"
        out[tag + "n_groups"] = np.int64(len(L.detect_labeling_groups(df, gap)) if len(df) else 0)
        for k, dt in (("group_id", np.int32), ("start_time", np.float64), ("end_time", np.float64),
                      ("duration", np.float64), ("s1_count", np.int32), ("avg_delta_t", np.float64),
                      ("avg_bpm", np.float64), ("pairs_count", np.int32)):
            out[tag + k] = np.asarray([s[k] for s in st], dt)
    if len(df):
        a, b, sel = L.calculate_avg_delta_t_in_range(df, df["Time (s)"].min(), df["Time (s)"].max())
    else:
        a, b, sel = None, None, []
    assert len(sel) == len(pairs)
    out["avg_delta_t"] = np.float64(np.nan if a is None else a)
    out["avg_bpm"] = np.float64(np.nan if b is None else b)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.mkdir("processed_files")
            L.save_labels(df, name)
            with open(os.path.join("processed_files", f"{name}_labels.csv"), "rb") as f:
                out["text"] = np.str_(f.read().decode("utf-8"))
            back = L.load_labels(name)
        finally:
            os.chdir(cwd)
    assert list(back.columns) == COLS and len(back) == len(df), name
    if len(df):
        assert list(back["Peak Type"]) == list(df["Peak Type"]), name
        # pandas' default parser may be an ulp off; the table itself is the definition
        np.testing.assert_allclose(back["Time (s)"].to_numpy(float), out["time"], rtol=1e-15, atol=0)
        np.testing.assert_allclose(back["Average BPM"].to_numpy(float), out["bpm"], rtol=1e-15, atol=0)
    return out


def csv_floats(text):
    T, B = [], []
    for ln in str(text).splitlines()[1:]:
        if ln.strip():
            a, b = ln.split(",")
            T.append(float(a))
            B.append(float(b))
    return np.asarray(T, np.float64), np.asarray(B, np.float64)


def golden_cases(L, PeakType, out_dir):
    n_with = 0
    for p in sorted(glob.glob(os.path.join(HERE, "beats", "*.npz"))):
        g = np.load(p)
        name = os.path.splitext(os.path.basename(p))[0]
        if "final_peaks" not in g.files:              # the reference raised: no beats, no labels
            np.savez_compressed(os.path.join(out_dir, name + ".npz"), none=np.bool_(True))
            print(f"{name}: none")
            continue
        raw, fin, sr = g["all_raw_peaks"].astype(np.int64), g["final_peaks"].astype(np.int64), int(g["sr"])
        info = dict(zip((int(k) for k in g["info_keys"]), (str(v) for v in g["info_vals"])))
        T, B = csv_floats(g["csv"]) if "csv" in g.files else (np.zeros(0), np.zeros(0))
        if len(fin) < 2 or len(T) == 0:
            np.savez_compressed(os.path.join(out_dir, name + ".npz"), none=np.bool_(True))
            print(f"{name}: none")
            continue
        infin = np.isin(raw, fin)
        types = np.array([1 if infin[i] else (2 if PeakType.is_s2(info.get(int(k), "")) else 0)
                          for i, k in enumerate(raw)], np.int8)
        dropped = sum(1 for i, k in enumerate(raw) if not infin[i] and PeakType.is_s1(info.get(int(k), "")))
        res = run_labeler(L, name, raw, types, sr, T, B)
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), none=np.bool_(False), types=types,
                            s1_string_not_final=np.int64(dropped), **res)
        n_with += 1
        print(f"{name}: {len(res['pos'])} labels, {len(res['pair_dt'])} pairs, groups at gap 1: "
              f"{int(res['g1_n_groups'])} ({len(res['g1_group_id'])} with statistics), "
              f"{dropped} S1 strings removed by the refinement")
    return n_with


def random_cases(L, out_dir, n_cases=48, seed=20240):
    rng = np.random.default_rng(seed)
    store = {"n_cases": np.int64(n_cases)}
    for c in range(n_cases):
        n = int(rng.integers(2, 40))
        if c % 6 == 0:                                # steps exactly at a threshold: 1, 3 and 5 s apart
            steps = rng.choice([250, 500, 1000, 3000, 5000], size=n)
        elif c % 6 == 1:                              # long pauses: several groups, some of a single S1
            steps = np.where(rng.random(n) < 0.3, rng.integers(900, 6000, n), rng.integers(150, 500, n))
        else:
            steps = rng.integers(1, 1500, n)
        raw = np.cumsum(steps).astype(np.int64)
        kind = c % 4
        if kind == 0:                                 # ragged
            types = rng.choice([0, 1, 2], size=n, p=[0.15, 0.45, 0.4]).astype(np.int8)
        elif kind == 1:                               # a run of S2 before the first S1
            types = rng.choice([1, 2], size=n).astype(np.int8)
            types[: min(n - 1, int(rng.integers(1, 6)))] = 2
        elif kind == 2:                               # alternating with holes
            types = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int8)
            types[rng.random(n) < 0.2] = 0
        else:                                         # mostly S1
            types = rng.choice([1, 2], size=n, p=[0.8, 0.2]).astype(np.int8)
        if c == 5:
            types[:] = 2                              # no S1 at all
        if c == 7:
            types[:] = 1                              # no S2 at all
        if c == 9:
            types[:] = 0                              # nothing labelled: the header line alone
        m = int(rng.integers(1, 30))
        if (types == 1).sum() >= 2:                   # a curve has fewer rows than there are beats
            m = min(m, int((types == 1).sum()) - 1)
        bt = np.sort(rng.integers(0, int(raw[-1]) + 2000, m)).astype(np.float64) / 1000.0
        if c % 5 == 0 and m > 2:
            bt[1] = bt[0]                             # equal times: the first of equal distances wins
        bv = np.round(rng.uniform(40, 220, m), 3)
        if c % 3 == 0:
            bv[rng.random(m) < 0.25] = np.nan
            if np.isnan(bv).all():
                bv[0] = 77.125
        keep = ~np.isnan(bv)
        T = np.array([float(f"{x:.3f}") for x in bt[keep]], np.float64)
        B = np.array([float(f"{x:.3f}") for x in bv[keep]], np.float64)
        res = run_labeler(L, f"random{c}", raw, types, 1000, T, B)
        store[f"c{c}_raw"], store[f"c{c}_types"], store[f"c{c}_bt"], store[f"c{c}_bv"] = raw, types, bt, bv
        for k, v in res.items():
            store[f"c{c}_{k}"] = v
    np.savez_compressed(os.path.join(out_dir, "_random.npz"), **store)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BPMX_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: make_label_goldens.py /path/to/reference")
    L, PeakType = _reference(ref)
    out_dir = os.path.join(HERE, "labels")
    os.makedirs(out_dir, exist_ok=True)
    n = golden_cases(L, PeakType, out_dir)
    random_cases(L, out_dir)
    print(f"{n} recordings with labels")


if __name__ == "__main__":
    main()
