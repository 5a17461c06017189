"""labels.rows_from_marks / labels.revise (the analysis of a person's corrected
marks on the host) against the fixtures of tests/golden/marks, which the
reference's own functions made from corrected label tables
(tests/golden/make_marks_goldens.py): curve, HRV table and record values bit
for bit, summary and CSV text, the re-stated label table with pairs, groups
and statistics, the file's bytes; the two rounding properties of the
re-stated times; the record identity; the rule's edge cases."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest

from bpm_analysis_amd import beats as B
from bpm_analysis_amd import labels as LB
from bpm_analysis_amd import reports as RP
from bpm_analysis_amd.config import DEFAULT_PARAMS
from tests import labels_cases as LC
from tests import marks_cases as MC
from tests import test_beats as TB

GOLD = os.path.join(TB.GOLD, "marks")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLD, "*.npz")))


def fixture(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    fx = {k: g[k] for k in g.files}
    params = dict(DEFAULT_PARAMS)
    params.update(json.loads(str(fx["params"])))
    table = LB._table([-1] * len(fx["c_type"]), fx["c_type"], fx["c_time"], np.full(len(fx["c_type"]), 60.0))
    return fx, params, table


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


def same_obj(ours, ref, what):
    """A stats dict against the fixture's: timestamps as nanoseconds, doubles as bit patterns."""
    if ref is None:
        assert ours is None, what
        return
    assert ours is not None and list(ours) == list(ref), what
    for k, v in ref.items():
        if isinstance(v, dict):
            assert pd.Timestamp(ours[k]).value == v["ns"], (what, k)
        else:
            assert bits(ours[k]) == bits(v), (what, k)


def assert_metrics(m, fx, where):
    """final_metrics against a fixture: curve, times, HRV frame and record values bit for bit."""
    assert bits(m["bpm_times"]) == bits(fx["bpm_times"]), where
    assert bits(m["smoothed_bpm"].values) == bits(fx["bpm_v"]), where
    h = m["windowed_hrv_df"]
    for c in ("time", "rmssdc", "sdnn", "bpm"):
        assert bits(h[c].to_numpy(float) if len(h) else np.zeros(0)) == bits(fx["hrv_" + c]), (where, c)
    ref = json.loads(str(fx["metrics"]))
    for k in ("major_inclines", "major_declines"):
        assert len(m[k]) == len(ref[k]), (where, k)
        for i, (o, r) in enumerate(zip(m[k], ref[k])):
            same_obj(o, r, (where, k, i))
    for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
        same_obj(m[k], ref[k], (where, k))
    assert list(m["hrv_summary"]) == list(ref["hrv_summary"]), where
    for k, v in ref["hrv_summary"].items():
        assert bits(m["hrv_summary"][k]) == bits(v), (where, k)


def test_fixtures_hold_every_kind_of_correction():
    assert len(NAMES) == 5
    merged = dropped = 0
    for name in NAMES:
        fx, _, table = fixture(name)
        rec = fx["record"]
        MC.check_identity(rec, len(LB.marks_from_table(table)["ms"]))
        merged += int(rec[LB.MK_N_MERGED])
        dropped += int(rec[LB.MK_N_DROPPED])
        assert (np.diff(fx["c_time"]) < 0).any()                              # a file need not be in order
        assert len(fx["bpm_v"]) > 0 and len(fx["pair_dt"]) > 0 and len(fx["hrv_time"]) > 0, name
    assert merged >= 5 and dropped >= 1
    # (no corrected curve here keeps a major decline: removed and added beats break the long falls up)
    kinds = {k: 0 for k in ("major_inclines", "hrr_stats", "peak_recovery_stats", "peak_exertion_stats")}
    for name in NAMES:
        for k, v in json.loads(str(fixture(name)[0]["metrics"])).items():
            if k in kinds and v:
                kinds[k] += 1
    assert all(kinds.values()), kinds


@pytest.mark.parametrize("name", NAMES)
def test_revise_equals_the_reference(name, tmp_path):
    fx, params, table = fixture(name)
    sr = int(fx["sr"])
    r = LB.revise(table, sr, params)
    assert r["status"] == LB.MARKS_OK and r["record"].tolist() == fx["record"].tolist()
    assert r["rows"]["idx"].tolist() == fx["row_idx"].tolist() and r["rows"]["type"].tolist() == fx["row_type"].tolist()
    assert r["final_peaks"].tolist() == fx["final_peaks"].tolist()
    assert_metrics(r["final_metrics"], fx, name)
    # summary and CSV byte-equal apart from the timestamp line
    fname = os.path.join(str(tmp_path), name + "_corrected.wav")
    assert TB._drop_stamp(RP.summary_text(fname, r["final_metrics"])) == str(fx["summary_md"])
    p = tmp_path / "bpm.csv"
    assert B.write_bpm_csv(str(p), r["final_metrics"]) is True
    assert p.read_bytes().decode("utf-8").replace("\r\n", "\n") == str(fx["csv"]).replace("\r\n", "\n")
    # the re-stated table, its pairs, groups and statistics, and the file's bytes
    for gap in LC.GAPS:
        got = LB.revise(table, sr, params, gap_sec=gap)["labels"]
        LC.assert_same(got, LC.expected(fx, gap), (name, gap))
    assert LB.labels_csv_text(r["labels"]).encode("utf-8") == str(fx["text"]).encode("utf-8")
    # a mark table and a label table give the same
    again = LB.revise(LB.marks_from_table(table), sr, params)
    assert LB.same(again["labels"], r["labels"]) and again["record"].tolist() == r["record"].tolist()


def test_revised_table_is_a_fixed_point():
    """The re-stated label file read back and revised again gives itself: every row is on the sample grid."""
    for name in NAMES:
        fx, params, table = fixture(name)
        sr = int(fx["sr"])
        first = LB.revise(table, sr, params)
        back = LB.parse_labels(LB.labels_csv_text(first["labels"]))
        second = LB.revise(back, sr, params)
        assert second["record"].tolist()[:3] == first["record"].tolist()[:3] and second["record"][3:].tolist() == [0] * 5
        assert LB.same(second["labels"], first["labels"]), name


@pytest.mark.parametrize("sr", [3, 16, 147, 302, 441, 999, 1000])
def test_time_round_trip_below_1000_hz(sr):
    """idx -> round(idx / sr, 3) -> ms -> idx is exact: any time the labeler or labels.py can have written for
    sr <= 1000 comes back as the sample it was."""
    idx = np.arange(120000, dtype=np.int64)
    t = np.array([round(i / sr, 3) for i in idx.tolist()])
    ms = LB._ms(t).astype(np.int64)
    assert ((ms * sr + 500) // 1000 == idx).all()
    rows = LB.rows_from_marks({"ms": ms[:5000], "type": np.full(5000, LB.S1)}, sr)
    assert rows["idx"].tolist() == idx[:5000].tolist() and rows["record"][LB.MK_N_MERGED] == 0


@pytest.mark.parametrize("sr", [1001, 2000, 2205, 44100, 48000])
def test_milliseconds_are_kept_above_1000_hz(sr):
    """ms is a fixed point of ms -> idx -> round(idx / sr, 3) * 1000: the person's own millisecond comes back."""
    ms = np.arange(60000, dtype=np.int64)
    idx = (ms * sr + 500) // 1000
    back = LB._ms(np.array([round(i / sr, 3) for i in idx.tolist()])).astype(np.int64)
    assert (back == ms).all()


def test_record_identity_and_statuses_on_the_shared_cases():
    seen = set()
    for c, w in zip(MC.cases(), MC.expected()):
        MC.check_identity(w["record"], len(c["ms"]))
        r = LB.revise(c, c["sr"], MC.params(), nd=c["nd"])
        assert r["status"] == w["status"] and r["record"].tolist() == w["record"].tolist(), c["name"]
        assert (r["final_metrics"] is None) == (w["status"] == LB.MARKS_FEW or "error" in r), c["name"]
        assert "error" not in r or isinstance(r["error"], ValueError), c["name"]
        if r["final_metrics"] is not None:
            assert bits(r["final_metrics"]["smoothed_bpm"].values) == bits(w["bpm"]), c["name"]
        seen.add(r["status"])
    assert seen == {LB.MARKS_OK, LB.MARKS_FEW}


def test_rule_on_small_tables():
    S1, S2 = LB.S1, LB.S2
    r = LB.rows_from_marks({"ms": [10, 10, 11, 20, 20], "type": [S2, S1, S2, S2, S2]}, 1000)
    assert r["idx"].tolist() == [10, 11, 20] and r["type"].tolist() == [S1, S2, S2] and r["record"].tolist() == \
        [3, 1, 2, 2, 0, 0, 0, 0]
    # a mark of another type between two on one sample does not split the run; a dropped one neither
    r = LB.rows_from_marks({"ms": [-1, 10, 10, 10], "type": [S1, S2, 0, S1]}, 1000)
    assert r["idx"].tolist() == [10] and r["type"].tolist() == [S1] and r["record"].tolist() == [1, 1, 0, 1, 1, 1, 0, 0]
    # half a sample rounds up: idx = (ms * sr + 500) // 1000
    assert LB.rows_from_marks({"ms": [166, 167, 500], "type": [S1, S1, S1]}, 3)["idx"].tolist() == [0, 1, 2]
    assert LB.rows_from_marks({"ms": [2 ** 31 - 1], "type": [S1]}, 1)["idx"].tolist() == [2147484]
    assert LB.rows_from_marks({"ms": [2 ** 31 - 1], "type": [S1]}, 1001)["record"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert LB.rows_from_marks(None, 147)["record"].tolist() == [0] * 8
    assert LB.rows_from_marks(LB.empty_table(), 147)["idx"].dtype == np.int64
    assert (LB.MARKS_FEW, LB.MARKS_OVERFLOW, LB.MARKS_RECORD) == (-24, -25, 8)
