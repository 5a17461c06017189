"""The labeler's output from the analysis' own decisions.

``heartbeat_labeler.py`` exists to produce ``<base>_labels.csv`` (a table of
S1 and S2 marks: time, average BPM, type) and the S1-S2 interval analysis
over that table: the S1->S2 pairs, the groups of marks separated by pauses and
per group the mean interval and BPM.  There a person clicks every mark.  Here
the marks are what the beat stages decided (line numbers: heartbeat_labeler.py):

* **S1**: every final beat (``final_peaks``, the beats behind ``_bpm_plot.csv``).
* **S2**: every raw peak that is not a final beat and whose final
  ``beat_debug_info`` string is an S2 (``PeakType.is_s2``: it starts with "S2").
* Nothing else is labelled; a peak whose string still says S1 but which the
  refinement removed gets no label.

A label row is what the labeler appends for a click exactly on the peak
(:530-546), ``x = idx / sr``: ``Time (s) = round(x, 3)`` (Python's ``round``,
the correctly rounded decimal, not numpy's multiply-rint-divide) and
``Average BPM = round(B[argmin |T - x|], 3)`` over the rows (T, B) of
``<base>_bpm_plot.csv`` as ``beats.write_bpm_csv`` writes them, each value
read back with ``float(text)``.  (The labeler reads that file with pandas'
default parser, which is not always correctly rounded; ``float`` is the
definition here.)

This module is the stage in plain Python on the host route's dicts
(``from_analysis``), the assembly of the device's slices (``assemble``:
``Detector.labels_device``, csrc/bpmx_labels_core.h states the same arithmetic
for the GPU) and the file: ``labels_csv_text`` gives the bytes the labeler's
``save_labels`` (:165-193) writes, ``read_labels`` / ``parse_labels`` restate
``load_labels`` (:118-163).

A result ("labels") is a dict:

* ``table``:  ``pos`` (position among the raw peaks), ``type`` (1 = S1, 2 = S2),
  ``time``, ``bpm``: one entry per label, ascending in time
* ``pairs``:  ``s1``, ``s2`` (label rows), ``dt`` (S2 time - S1 time, unrounded)
* ``groups``: the groups that have statistics: ``id`` (may jump), ``first``,
  ``last`` (label rows of the first and last S1), ``s1_count``, ``pairs_count``,
  ``avg_delta_t``, ``avg_bpm``
* ``summary``: ``n_labels``, ``n_s1``, ``n_s2``, ``n_pairs``, ``avg_delta_t``,
  ``avg_bpm`` (None without pairs)
* ``gap_sec``: the group threshold

The last part scores such a table against a person's corrected label file
(``marks_from_table``, ``score``, ``score_summary``, ``score_csv_text``): the
definition of ``Detector.score_device`` (bpmx_score_device) in plain Python.
After it, ``rows_from_marks`` and ``revise`` turn a corrected table into beats
and analyse those: the definition of ``Detector.marks_device``
(bpmx_marks_device) and the host route behind it.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np

S1, S2 = 1, 2
TYPE_NAME = {S1: "S1", S2: "S2"}
COLUMNS = ("Time (s)", "Average BPM", "Peak Type")
PAIR_COLUMNS = ("S1_Time", "S2_Time", "Delta_t", "S1_BPM")
HEADER = ",".join(COLUMNS) + "\n"
GAP_PASSES = 5
_TAG_S2 = 2             # bpmx_beat_tag
_GAP_S1, _GAP_S2 = 1, 2  # bpmx_trace_gap


# ---------------------------------------------------------------- which peaks, which type
def types_from_strings(raw_peaks, final_peaks, info: Dict) -> np.ndarray:
    """0 / S1 / S2 per raw peak from the final ``beat_debug_info`` strings."""
    raw = np.asarray(raw_peaks, dtype=np.int64)
    fin = np.isin(raw, np.asarray(final_peaks, dtype=np.int64))
    out = np.zeros(len(raw), np.int8)
    for i, p in enumerate(raw.tolist()):
        if fin[i]:
            out[i] = S1
        elif str(info.get(p, "")).strip().startswith("S2"):
            out[i] = S2
    return out


def types_from_tags(raw_peaks, final_peaks, tags, gap) -> np.ndarray:
    """The same from the device's numbers: the highest gap-fill pass that
    labelled the peak decides (the outermost ``ORIGINAL_REASON`` wrapper of
    ``explain.apply_gap_history``), else the main pass' tag."""
    raw = np.asarray(raw_peaks, dtype=np.int64)
    fin = np.isin(raw, np.asarray(final_peaks, dtype=np.int64))
    out = np.zeros(len(raw), np.int8)
    for i, (t, g) in enumerate(zip(np.asarray(tags).tolist(), np.asarray(gap).tolist())):
        if fin[i]:
            out[i] = S1
            continue
        top = 0
        for it in range(GAP_PASSES):
            v = (int(g) >> (2 * it)) & 3
            if v:
                top = v
        if (top == _GAP_S2) if top else (t == _TAG_S2):
            out[i] = S2
    return out


# ---------------------------------------------------------------- the table
def csv_rows(bpm_times, bpm):
    """(T, B): the rows of ``<base>_bpm_plot.csv`` read back with ``float``."""
    T, B = [], []
    for x, b in zip(np.asarray(bpm_times, dtype=np.float64).tolist(), np.asarray(bpm, dtype=np.float64).tolist()):
        if b == b:
            T.append(float(f"{x:.3f}"))
            B.append(float(f"{b:.3f}"))
    return np.asarray(T, dtype=np.float64), np.asarray(B, dtype=np.float64)


def _table(pos, typ, time, bpm) -> Dict:
    return {"pos": np.asarray(pos, dtype=np.int64), "type": np.asarray(typ, dtype=np.int8),
            "time": np.asarray(time, dtype=np.float64), "bpm": np.asarray(bpm, dtype=np.float64)}


def label_table(raw_peaks, types, sr: int, T, B) -> Dict:
    """The label rows of the typed raw peaks (:530-546), in table order."""
    raw = np.asarray(raw_peaks, dtype=np.int64)
    pos, typ, time, bpm = [], [], [], []
    for i in np.flatnonzero(np.asarray(types)).tolist():
        x = float(raw[i]) / float(sr)
        k = int(np.abs(T - x).argmin())               # find_nearest_idx: the first minimum
        pos.append(i)
        typ.append(int(types[i]))
        time.append(round(x, 3))
        bpm.append(round(float(B[k]), 3))
    return _table(pos, typ, time, bpm)


def empty_table() -> Dict:
    return _table([], [], [], [])


# ---------------------------------------------------------------- pairs, groups, statistics
def s1_s2_pairs(table: Dict) -> Dict:
    """``calculate_s1_s2_diffs`` (:198-217): the greedy walk over the S1 and S2
    rows with the strict ``>``."""
    typ, t = table["type"], table["time"].tolist()
    a, b = np.flatnonzero(typ == S1).tolist(), np.flatnonzero(typ == S2).tolist()
    s1, s2, dt = [], [], []
    i = j = 0
    while i < len(a) and j < len(b):
        if t[b[j]] > t[a[i]]:
            s1.append(a[i])
            s2.append(b[j])
            dt.append(t[b[j]] - t[a[i]])
            i += 1
        j += 1
    return {"s1": np.asarray(s1, dtype=np.int32), "s2": np.asarray(s2, dtype=np.int32),
            "dt": np.asarray(dt, dtype=np.float64)}


def groups(table: Dict, gap_sec: float = 5.0) -> List[tuple]:
    """``detect_labeling_groups`` (:244-276): (first S1 row, last S1 row, S1
    count) per group; the S1 marks are split where the step is >= gap."""
    a = np.flatnonzero(table["type"] == S1).tolist()
    if len(a) < 2:
        return []
    t = table["time"].tolist()
    out = [[a[0], a[0], 1]]
    for p, k in zip(a, a[1:]):
        if t[k] - t[p] < gap_sec:
            out[-1][1] = k
            out[-1][2] += 1
        else:
            out.append([k, k, 1])
    return [tuple(g) for g in out]


def _mean(values: List[float]) -> float:
    """``sum(list) / len(list)``: added left to right from 0."""
    s = 0
    for v in values:
        s = s + v
    return s / len(values)


def group_statistics(table: Dict, pairs: Dict, grps: List[tuple]) -> Dict:
    """``calculate_group_statistics`` (:278-308): a group of fewer than two S1
    marks, or without a pair whose S1 time lies in [start, end], is skipped but
    keeps its number."""
    t, b = table["time"].tolist(), table["bpm"].tolist()
    ps1, dts = pairs["s1"].tolist(), pairs["dt"].tolist()
    rows = []
    for g, (first, last, cnt) in enumerate(grps):
        if cnt < 2:
            continue
        sel = [p for p in range(len(ps1)) if t[first] <= t[ps1[p]] <= t[last]]
        if not sel:
            continue
        rows.append((g + 1, first, last, cnt, len(sel), _mean([dts[p] for p in sel]), _mean([b[ps1[p]] for p in sel])))
    cols = list(zip(*rows)) if rows else [[]] * 7
    i32 = lambda v: np.asarray(v, dtype=np.int32)  # noqa: E731
    return {"id": i32(cols[0]), "first": i32(cols[1]), "last": i32(cols[2]), "s1_count": i32(cols[3]),
            "pairs_count": i32(cols[4]), "avg_delta_t": np.asarray(cols[5], dtype=np.float64),
            "avg_bpm": np.asarray(cols[6], dtype=np.float64)}


def group_records(labels: Dict) -> List[Dict]:
    """The list of dicts ``calculate_group_statistics`` returns."""
    t, g = labels["table"]["time"], labels["groups"]
    out = []
    for k in range(len(g["id"])):
        start, end = float(t[g["first"][k]]), float(t[g["last"][k]])
        out.append({"group_id": int(g["id"][k]), "start_time": start, "end_time": end, "duration": end - start,
                    "s1_count": int(g["s1_count"][k]), "avg_delta_t": float(g["avg_delta_t"][k]),
                    "avg_bpm": float(g["avg_bpm"][k]), "pairs_count": int(g["pairs_count"][k])})
    return out


def summary(table: Dict, pairs: Dict) -> Dict:
    """Counts, and ``calculate_avg_delta_t_in_range`` over the whole table."""
    n = len(pairs["dt"])
    b = table["bpm"].tolist()
    return {"n_labels": len(table["type"]), "n_s1": int((table["type"] == S1).sum()),
            "n_s2": int((table["type"] == S2).sum()), "n_pairs": n,
            "avg_delta_t": _mean(pairs["dt"].tolist()) if n else None,
            "avg_bpm": _mean([b[k] for k in pairs["s1"].tolist()]) if n else None}


def analyse(table: Dict, gap_sec: float = 5.0) -> Dict:
    """Pairs, groups and summary of a label table."""
    p = s1_s2_pairs(table)
    return {"table": table, "pairs": p, "groups": group_statistics(table, p, groups(table, gap_sec)),
            "summary": summary(table, p), "gap_sec": float(gap_sec)}


# ---------------------------------------------------------------- from the two routes
def from_curve(raw_peaks, types, sr: int, bpm_times, bpm, gap_sec: float = 5.0) -> Optional[Dict]:
    T, B = csv_rows(bpm_times, bpm)
    if len(T) == 0:
        return None
    return analyse(label_table(raw_peaks, types, sr, T, B), gap_sec)


def from_analysis(res: Dict, sr: int, gap_sec: float = 5.0) -> Optional[Dict]:
    """The labels of one recording from the host route's dict
    (``beats.analyze_recording``: final_peaks, all_raw_peaks, analysis_data,
    final_metrics) or the device route's (``Beats.to_host(explain=True)``:
    final_peaks, raw_peaks, analysis_data, bpm_times, bpm).  None where there
    are none: an error, fewer than two final beats, a curve without a row that
    is not NaN."""
    if "error" in res or res.get("skipped") or "final_peaks" not in res or len(res["final_peaks"]) < 2:
        return None
    raw = res["all_raw_peaks"] if "all_raw_peaks" in res else res["raw_peaks"]
    m = res.get("final_metrics")
    if m is not None:
        bt, bv = m["bpm_times"], m["smoothed_bpm"].values
    elif "bpm" in res:
        bt, bv = res["bpm_times"], res["bpm"]
    else:
        return None
    types = types_from_strings(raw, res["final_peaks"], res["analysis_data"].get("beat_debug_info", {}))
    return from_curve(raw, types, sr, bt, bv, gap_sec)


def assemble(dev: Dict, gap_sec: float = 5.0) -> Dict:
    """A labels dict from one recording's device slices (``Labels.to_host``):
    ``lb_*`` [n_labels], ``pr_*`` [n_pairs], ``gr_*`` [n_groups] and the
    4-double ``record``."""
    rec = dev["record"]
    n = len(dev["pr_dt"])
    tab = _table(dev["lb_pos"], dev["lb_type"], dev["lb_time"], dev["lb_bpm"])
    return {"table": tab,
            "pairs": {"s1": np.asarray(dev["pr_s1"], np.int32), "s2": np.asarray(dev["pr_s2"], np.int32),
                      "dt": np.asarray(dev["pr_dt"], np.float64)},
            "groups": {"id": np.asarray(dev["gr_id"], np.int32), "first": np.asarray(dev["gr_first"], np.int32),
                       "last": np.asarray(dev["gr_last"], np.int32), "s1_count": np.asarray(dev["gr_s1"], np.int32),
                       "pairs_count": np.asarray(dev["gr_pairs"], np.int32),
                       "avg_delta_t": np.asarray(dev["gr_dt"], np.float64),
                       "avg_bpm": np.asarray(dev["gr_bpm"], np.float64)},
            "summary": {"n_labels": len(tab["type"]), "n_s1": int(rec[2]), "n_s2": int(rec[3]), "n_pairs": n,
                        "avg_delta_t": float(rec[0]) if n else None, "avg_bpm": float(rec[1]) if n else None},
            "gap_sec": float(gap_sec)}


def same(a: Optional[Dict], b: Optional[Dict]) -> bool:
    """Two labels dicts are equal: integers equal, doubles bit for bit."""
    if a is None or b is None:
        return a is None and b is None
    for part in ("table", "pairs", "groups"):
        if list(a[part]) != list(b[part]):
            return False
        for k in a[part]:
            x, y = np.asarray(a[part][k]), np.asarray(b[part][k])
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                return False
    sa, sb = a["summary"], b["summary"]
    if list(sa) != list(sb):
        return False
    for k in sa:
        if (sa[k] is None) != (sb[k] is None):
            return False
        if sa[k] is not None and np.float64(sa[k]).tobytes() != np.float64(sb[k]).tobytes():
            return False
    return a["gap_sec"] == b["gap_sec"]


# ---------------------------------------------------------------- the file
def labels_csv_text(labels: Optional[Dict]) -> str:
    """The text ``save_labels`` (:165-193) writes for the table: with pairs
    the two sections, the intervals after ``DataFrame.round(3)`` (numpy's
    rounding, only here); without pairs the plain table; an empty table (or
    None) the header line alone.  Floats as ``DataFrame.to_csv`` writes them:
    the shortest text that reads back the same."""
    if labels is None or len(labels["table"]["type"]) == 0:
        return HEADER
    tab, p = labels["table"], labels["pairs"]
    t, b = tab["time"].tolist(), tab["bpm"].tolist()
    rows = "".join(f"{repr(x)},{repr(v)},{TYPE_NAME[int(k)]}\n" for x, v, k in zip(t, b, tab["type"].tolist()))
    if len(p["dt"]) == 0:
        return HEADER + rows
    cols = np.round(np.array([tab["time"][p["s1"]], tab["time"][p["s2"]], p["dt"], tab["bpm"][p["s1"]]]), 3)
    pairs = "".join(",".join(repr(v) for v in r) + "\n" for r in cols.T.tolist())
    return "# Peak Labels\n" + HEADER + rows + "\n# S1-S2 Intervals\n" + ",".join(PAIR_COLUMNS) + "\n" + pairs


def labels_path(original_file_path: str, output_directory: str) -> str:
    base = os.path.basename(os.path.splitext(original_file_path)[0])
    return os.path.join(output_directory, f"{base}_labels.csv")


def write_labels(path: str, labels: Optional[Dict], overwrite: bool = False) -> bool:
    """Write ``<base>_labels.csv``.  That file is where the labeler keeps hand
    labels: an existing one is left as it is (False) unless `overwrite`."""
    if os.path.exists(path) and not overwrite:
        return False
    with open(path, "w", newline="", encoding="utf-8") as f:
        f.write(labels_csv_text(labels))
    return True


def parse_labels(content: str) -> Dict:
    """The label table of a label file's text in either format (the sections,
    or the plain table), numbers read with ``float``.  ``pos`` is -1: a file
    does not say which raw peak a row came from."""
    lines = content.split("\n")
    if "# Peak Labels" in content:
        start = end = None
        for i, line in enumerate(lines):
            if line.strip() == "# Peak Labels":
                start = i + 1
            elif line.strip() == "# S1-S2 Intervals" and start is not None:
                end = i
                break
        if start is not None:
            lines = lines[start:end]
    names = {v: k for k, v in TYPE_NAME.items()}
    typ, time, bpm = [], [], []
    cols = None
    for row in (ln for ln in lines if ln.strip()):
        cells = row.split(",")
        if cols is None:
            cols = [cells.index(c) for c in COLUMNS]
            continue
        time.append(float(cells[cols[0]]))
        bpm.append(float(cells[cols[1]]))
        typ.append(names[cells[cols[2]].strip()])
    return _table([-1] * len(typ), typ, time, bpm)


def read_labels(path: str) -> Dict:
    """``load_labels`` (:118-163): the label table of ``<base>_labels.csv``
    (``parse_labels``).  A missing file is an empty table, as there."""
    if not os.path.exists(path):
        return empty_table()
    with open(path, "r", encoding="utf-8") as f:
        return parse_labels(f.read())


# ---------------------------------------------------------------- scoring against corrected labels
# There is no reference implementation of scoring: include/bpmx.h (bpmx_score_device) is the definition,
# csrc/bpmx_score_core.h states it for host and device, and this is the same in plain Python.
SCORE_OK, SCORE_NO_LABELS, SCORE_NONE, SCORE_OVERFLOW = 0, 1, -22, -23       # bpmx_score_status
KIND_OUTSIDE, KIND_TP, KIND_SWAP, KIND_FP, KIND_FN = 0, 1, 2, 3, 3            # bpmx_score_kind
KIND_NAME = {KIND_OUTSIDE: "OUTSIDE", KIND_TP: "TP", KIND_SWAP: "SWAP", KIND_FP: "FP"}
# bpmx_score_record: nine fields per type (S1, then S2), then two for the file
SR_N_REF, SR_N_DET, SR_TP, SR_SWAP, SR_FP, SR_FN, SR_SUM_ERR, SR_SUM_ABS, SR_MAX_ABS = range(9)
SR_PER_TYPE, SR_N_OUTSIDE, SR_N_SPANS, SCORE_RECORD = 9, 18, 19, 20
SCORE_COLUMNS = ("Time (s)", "Peak Type", "Kind", "Partner Time (s)")
_I32 = (-2 ** 31, 2 ** 31 - 1)


def _ms(times) -> np.ndarray:
    """Integer milliseconds: one multiplication, round to nearest even, saturated to int32."""
    q = np.rint(np.asarray(times, dtype=np.float64) * 1000.0)
    q = np.where(np.isnan(q), _I32[0], q)
    return np.clip(q, _I32[0], _I32[1]).astype(np.int64).astype(np.int32)


def score_ms(tol_sec: float, gap_sec: float):
    """(tol_ms, gap_ms) of the two thresholds in seconds; ValueError unless
    tol_ms >= 0 and gap_ms > 2 * tol_ms (the labelled spans must stay apart)."""
    tol, gap = int(round(float(tol_sec) * 1000)), int(round(float(gap_sec) * 1000))
    if tol < 0 or gap <= 2 * tol or gap > _I32[1]:
        raise ValueError(f"score: needs tol_ms >= 0 and gap_ms > 2 * tol_ms (got {tol}, {gap})")
    return tol, gap


def marks_from_table(table: Optional[Dict]) -> Dict:
    """The reference marks of a corrected label table (``read_labels``), as
    they are uploaded: rows whose type is neither S1 nor S2 or whose time is
    NaN dropped (``dropped`` counts them), ``ms = int(np.rint(time * 1000.0))``,
    sorted stably by ms.  ``row`` is each mark's row in `table`."""
    if table is None:
        table = empty_table()
    typ = np.asarray(table["type"]).astype(np.int64)
    t = np.asarray(table["time"], dtype=np.float64)
    keep = np.flatnonzero(((typ == S1) | (typ == S2)) & ~np.isnan(t))
    ms = _ms(t[keep])
    order = np.argsort(ms, kind="stable")
    return {"ms": ms[order], "type": typ[keep][order].astype(np.int32), "time": t[keep][order],
            "row": keep[order].astype(np.int64), "dropped": int(len(typ) - len(keep))}


def _walk(D: List[tuple], R: List[tuple], tol: int) -> List[tuple]:
    """The walk over two ascending lists of (ms, row): within `tol` a match,
    else the smaller one steps.  A maximum matching for a symmetric tolerance."""
    i = j = 0
    out = []
    while i < len(R) and j < len(D):
        if abs(D[j][0] - R[i][0]) <= tol:
            out.append((D[j][1], R[i][1]))
            i += 1
            j += 1
        elif D[j][0] < R[i][0]:
            j += 1
        else:
            i += 1
    return out


def score(table: Optional[Dict], ref_table: Optional[Dict], tol_sec: float = 0.05, gap_sec: float = 5.0) -> Dict:
    """The detected marks of one recording (`table`: a labels dict's
    ``table``, or None where the analysis made no labels) scored against a
    person's corrected marks (`ref_table`: a label table, or the dict of
    ``marks_from_table``).

    Labelled spans: the reference marks of both types together; a new span
    starts where the step is >= gap; a span is [first - tol, last + tol].  A
    detected mark in no span is outside.  Pass 1, per type: the walk of the
    in-span detected marks against the reference marks of the type: TP.  Pass
    2, per type: the detected marks left against the reference marks of the
    other type left: SWAP.  What is left: FP (detected), FN (reference).

    Returns ``record`` (int64[20], ``SR_*``), ``status`` and the rows
    ``sc_kind`` / ``sc_ref`` per detected mark and ``rf_kind`` / ``rf_det``
    per reference mark (int32; empty with ``SCORE_NONE``: no reference mark),
    plus ``marks`` and ``det_ms``."""
    tol, gap = score_ms(tol_sec, gap_sec)
    marks = ref_table if ref_table is not None and "ms" in ref_table else marks_from_table(ref_table)
    status = SCORE_OK if table is not None else SCORE_NO_LABELS
    dms = _ms(table["time"]).tolist() if table is not None else []
    dty = np.asarray(table["type"]).astype(np.int64).tolist() if table is not None else []
    rms, rty = marks["ms"].tolist(), marks["type"].tolist()
    nd, nr = len(dms), len(rms)
    rec = np.zeros(SCORE_RECORD, np.int64)
    e32 = np.zeros(0, np.int32)
    out = {"record": rec, "status": status, "sc_kind": e32, "sc_ref": e32, "rf_kind": e32, "rf_det": e32,
           "marks": marks, "det_ms": np.asarray(dms, np.int32), "tol_ms": tol, "gap_ms": gap}
    if nr == 0:
        rec[SR_N_OUTSIDE] = nd
        out["status"] = SCORE_NONE
        return out
    spans = []
    for i, m in enumerate(rms):
        if i == 0 or m - rms[i - 1] >= gap:
            spans.append([m, m])
        spans[-1][1] = m
    inside = [any(a - tol <= d <= z + tol for a, z in spans) for d in dms]
    sc_kind = [KIND_FP if inside[j] and dty[j] in (S1, S2) else KIND_OUTSIDE for j in range(nd)]
    rf_kind = [KIND_FN if rty[i] in (S1, S2) else KIND_OUTSIDE for i in range(nr)]
    sc_ref, rf_det = [-1] * nd, [-1] * nr
    for kind in (KIND_TP, KIND_SWAP):
        for k, typ in enumerate((S1, S2)):
            other = typ if kind == KIND_TP else (S2 if typ == S1 else S1)
            D = [(dms[j], j) for j in range(nd) if sc_kind[j] == KIND_FP and dty[j] == typ]
            R = [(rms[i], i) for i in range(nr) if rf_kind[i] == KIND_FN and rty[i] == other]
            for j, i in _walk(D, R, tol):
                sc_kind[j], sc_ref[j], rf_kind[i], rf_det[i] = kind, i, kind, j
                if kind == KIND_TP:
                    e = dms[j] - rms[i]
                    r = rec[k * SR_PER_TYPE:]
                    r[SR_SUM_ERR] += e
                    r[SR_SUM_ABS] += abs(e)
                    r[SR_MAX_ABS] = max(int(r[SR_MAX_ABS]), abs(e))
    for k, typ in enumerate((S1, S2)):
        r = rec[k * SR_PER_TYPE:]
        mine = [sc_kind[j] for j in range(nd) if dty[j] == typ and sc_kind[j] != KIND_OUTSIDE]
        theirs = [rf_kind[i] for i in range(nr) if rty[i] == typ]
        r[SR_N_REF], r[SR_N_DET] = len(theirs), len(mine)
        r[SR_TP], r[SR_SWAP], r[SR_FP] = mine.count(KIND_TP), mine.count(KIND_SWAP), mine.count(KIND_FP)
        r[SR_FN] = theirs.count(KIND_FN)
    rec[SR_N_OUTSIDE] = sc_kind.count(KIND_OUTSIDE)
    rec[SR_N_SPANS] = len(spans)
    out.update(sc_kind=np.asarray(sc_kind, np.int32), sc_ref=np.asarray(sc_ref, np.int32),
               rf_kind=np.asarray(rf_kind, np.int32), rf_det=np.asarray(rf_det, np.int32))
    return out


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def score_summary(record) -> Dict:
    """Precision, recall, F1 and the mean errors in seconds from one integer
    record (a file's, or the sum of many files' with ``MAX_ABS`` their
    maximum: ``score_total``).  Per type (``"S1"``, ``"S2"``) and ``"all"``
    (both types added); ``n_outside`` and ``n_spans``.  A division by zero
    gives NaN."""
    rec = np.asarray(record, dtype=np.int64).reshape(SCORE_RECORD)
    parts = {"S1": rec[:SR_PER_TYPE], "S2": rec[SR_PER_TYPE:2 * SR_PER_TYPE]}
    both = parts["S1"] + parts["S2"]
    both[SR_MAX_ABS] = max(int(parts["S1"][SR_MAX_ABS]), int(parts["S2"][SR_MAX_ABS]))
    parts["all"] = both
    out: Dict = {"n_outside": int(rec[SR_N_OUTSIDE]), "n_spans": int(rec[SR_N_SPANS])}
    for name, r in parts.items():
        tp = int(r[SR_TP])
        p, q = _ratio(tp, r[SR_N_DET]), _ratio(tp, r[SR_N_REF])
        f1 = 2 * p * q / (p + q) if p + q > 0 else (float("nan") if p != p or q != q else 0.0)
        out[name] = {"n_ref": int(r[SR_N_REF]), "n_det": int(r[SR_N_DET]), "tp": tp, "swap": int(r[SR_SWAP]),
                     "fp": int(r[SR_FP]), "fn": int(r[SR_FN]), "precision": p, "recall": q, "f1": f1,
                     "mean_err_sec": _ratio(r[SR_SUM_ERR], tp) / 1000.0,
                     "mean_abs_err_sec": _ratio(r[SR_SUM_ABS], tp) / 1000.0,
                     "max_abs_err_sec": float(r[SR_MAX_ABS]) / 1000.0 if tp else float("nan")}
    return out


def score_total(records) -> np.ndarray:
    """The record of many files: every field added, ``MAX_ABS`` the maximum."""
    r = np.asarray(records, dtype=np.int64).reshape(-1, SCORE_RECORD)
    tot = r.sum(axis=0)
    for k in (SR_MAX_ABS, SR_PER_TYPE + SR_MAX_ABS):
        tot[k] = r[:, k].max() if len(r) else 0
    return tot


def score_csv_text(table: Optional[Dict], result: Dict) -> str:
    """The list of mistakes of one recording: one row per mark that is not a
    TP, ascending in time: the detected marks outside every span, swapped and
    false (``OUTSIDE``, ``SWAP``, ``FP``) and the reference marks missed
    (``FN``), with the partner's time for a SWAP.  `result`: ``score``'s dict,
    or ``Scores.to_host``'s with ``marks``."""
    marks = result["marks"]
    rows = []
    if table is not None and len(result["sc_kind"]):
        for j, (t, k) in enumerate(zip(np.asarray(table["time"]).tolist(), np.asarray(table["type"]).tolist())):
            kind, i = int(result["sc_kind"][j]), int(result["sc_ref"][j])
            if kind != KIND_TP:
                rows.append((t, 0, f"{repr(t)},{TYPE_NAME.get(int(k), k)},{KIND_NAME[kind]},"
                                   f"{repr(float(marks['time'][i])) if i >= 0 else ''}\n"))
    for i, kind in enumerate(np.asarray(result["rf_kind"]).tolist()):
        if kind == KIND_FN:
            t = float(marks["time"][i])
            rows.append((t, 1, f"{repr(t)},{TYPE_NAME[int(marks['type'][i])]},FN,\n"))
    rows.sort(key=lambda r: (r[0], r[1]))
    return ",".join(SCORE_COLUMNS) + "\n" + "".join(r[2] for r in rows)


# ---------------------------------------------------------------- corrected marks as beats
# There is no reference implementation of the conversion: include/bpmx.h (bpmx_marks_device) is the definition,
# csrc/bpmx_marks_core.h states it for host and device, and this is the same in numpy.
MARKS_OK, MARKS_FEW, MARKS_OVERFLOW = 0, -24, -25                             # bpmx_marks_status
MK_N_ROWS, MK_N_S1, MK_N_S2, MK_N_MERGED, MK_N_DROPPED, MK_N_OTHER, MARKS_RECORD = 0, 1, 2, 3, 4, 5, 8


def rows_from_marks(marks: Optional[Dict], sr: int, nd: Optional[int] = None) -> Dict:
    """The rows of a person's marks (``marks_from_table``'s dict, or a label
    table, which goes through it; any dict with ``ms`` and ``type``) at the
    decimated rate `sr`, integers only: a mark whose type is neither S1 nor
    S2 is skipped, one with ``ms < 0``, ``idx = (ms * sr + 500) // 1000 >
    INT32_MAX`` or (with `nd`) ``idx >= nd`` is dropped, a run of kept marks
    on one sample becomes one row, S1 if any of them is.  Returns ``idx``
    (int64), ``type`` (int8), ``final`` (the S1 rows' idx) and ``record``
    (int32 [8]: rows, S1, S2, merged, dropped, other, 0, 0).  Times are
    restated as ``round(idx / sr, 3)``: a time off the sample grid snaps to
    the nearest sample."""
    if marks is None or "ms" not in marks:
        marks = marks_from_table(marks)
    ms = np.asarray(marks["ms"]).astype(np.int64)
    typ = np.asarray(marks["type"]).astype(np.int64)
    typed = (typ == S1) | (typ == S2)
    idx = (np.maximum(ms, 0) * int(sr) + 500) // 1000
    ok = (ms >= 0) & (idx <= _I32[1])
    if nd is not None:
        ok &= idx < int(nd)
    keep = typed & ok
    ki, kt = idx[keep], typ[keep]
    head = np.ones(len(ki), dtype=bool)
    head[1:] = ki[1:] != ki[:-1]
    starts = np.flatnonzero(head)
    any_s1 = np.logical_or.reduceat(kt == S1, starts) if len(starts) else np.zeros(0, dtype=bool)
    r_idx, r_type = ki[head], np.where(any_s1, S1, S2).astype(np.int8)
    rec = np.zeros(MARKS_RECORD, dtype=np.int32)
    rec[MK_N_ROWS], rec[MK_N_S1] = len(r_idx), int(any_s1.sum())
    rec[MK_N_S2] = rec[MK_N_ROWS] - rec[MK_N_S1]
    rec[MK_N_MERGED] = len(ki) - len(r_idx)
    rec[MK_N_DROPPED] = int((typed & ~ok).sum())
    rec[MK_N_OTHER] = int((~typed).sum())
    return {"idx": r_idx.astype(np.int64), "type": r_type, "final": r_idx[r_type == S1].astype(np.int64), "record": rec}


def revise(table_or_marks: Optional[Dict], sr: int, params: Dict, gap_sec: float = 5.0,
           nd: Optional[int] = None) -> Dict:
    """The analysis of a person's own marks on the host: ``rows_from_marks``,
    ``beats.final_metrics`` on the S1 indices (curve, HRV table, HRR, slopes,
    inclines and declines, summary) and ``from_curve`` on the rows, so the
    label table's ``Average BPM`` and the group statistics follow the
    corrected curve.  Returns ``rows``, ``record``, ``final_peaks``,
    ``status`` (MARKS_OK, or MARKS_FEW with fewer than two S1 rows),
    ``final_metrics`` and ``labels`` (both None with MARKS_FEW; ``labels``
    also where the curve has no row; ``final_metrics`` also where scipy's
    find_peaks rejects the curve's spacing, with the ValueError as ``error``,
    as ``Metrics.to_host`` reports it)."""
    from . import beats as B
    rows = rows_from_marks(table_or_marks, sr, nd)
    out = {"rows": rows, "record": rows["record"], "final_peaks": rows["final"], "status": MARKS_FEW,
           "final_metrics": None, "labels": None}
    if len(rows["final"]) >= 2:
        out["status"] = MARKS_OK
        try:
            out["final_metrics"] = B.final_metrics(rows["final"], int(sr), params)
        except ValueError as e:                       # scipy's, where the curve is too dense for find_peaks' distance
            out["error"] = e
        s, t = B.bpm_series(rows["final"], int(sr), params)
        out["labels"] = from_curve(rows["idx"], rows["type"], int(sr), t, s.values, gap_sec) if len(s) else None
    return out
