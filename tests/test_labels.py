"""bpm_analysis_amd/labels.py against the fixtures of tests/golden/labels,
which the reference labeler's own functions made (find_nearest_idx,
calculate_s1_s2_diffs, detect_labeling_groups, calculate_group_statistics,
calculate_avg_delta_t_in_range, save_labels, load_labels): table, pairs,
groups, summary and the file's bytes; the read_labels round trip, the
overwrite rule, the empty and pair-less file forms."""
import os

import numpy as np
import pytest

from bpm_analysis_amd import beats as B
from bpm_analysis_amd import labels as LB
from tests import labels_cases as LC
from tests import test_beats as TB


def test_fixtures_are_what_the_issue_counts():
    fx = [(n, f) for n, f, _ in LC.golden_cases()]
    none = sorted(n for n, f in fx if bool(f["none"]))
    assert none == ["ref_44k_10s_zeros", "ref_44k_short16"] and len(fx) - len(none) == 26
    pairs = {n: len(f["pair_dt"]) for n, f in fx if not bool(f["none"])}
    assert [n for n, v in pairs.items() if v == 0] == ["env_static_fallback"] and max(pairs.values()) == 930
    clicks = LC.fixture("ref_44k_40s_clicks")
    assert int(clicks["g1_n_groups"]) == 6 and len(clicks["g1_group_id"]) == 5
    assert int(LC.fixture("env_plateaus")["s1_string_not_final"]) == 19 and int(clicks["s1_string_not_final"]) == 3
    assert len(LC.random_cases()) >= 36


@pytest.mark.parametrize("gap", LC.GAPS)
def test_golden_tables(gap):
    for name, fx, c in LC.golden_cases():
        want = LC.expected(fx, gap)
        got = None if c is None else LC.host(c, gap)
        LC.assert_same(got, want, (name, gap))
        if want is not None:
            # the CSV rows are beats.write_bpm_csv's, read with float
            g = np.load(os.path.join(TB.GOLD, "beats", name + ".npz"))
            T, Bv = LB.csv_rows(c["bt"], c["bv"])
            rows = [ln.split(",") for ln in str(g["csv"]).splitlines()[1:] if ln.strip()]
            assert T.tolist() == [float(a) for a, _ in rows] and Bv.tolist() == [float(b) for _, b in rows], name
            recs = LB.group_records(got)
            tag = f"g{gap}_"
            assert [r["duration"] for r in recs] == fx[tag + "duration"].tolist(), name
            assert [r["start_time"] for r in recs] == fx[tag + "start_time"].tolist(), name
            assert [r["end_time"] for r in recs] == fx[tag + "end_time"].tolist(), name


@pytest.mark.parametrize("gap", LC.GAPS)
def test_random_tables(gap):
    jumps = single = before = 0
    for name, fx, c in LC.random_cases():
        got = LB.from_curve(c["raw"], c["types"], 1000, c["bt"], c["bv"], gap)
        LC.assert_same(got, LC.expected(fx, gap), (name, gap))
        ids = got["groups"]["id"]
        jumps += len(ids) > 0 and (ids[0] != 1 or (np.diff(ids) > 1).any())
        single += any(n == 1 for _, _, n in LB.groups(got["table"], gap))
        t = got["table"]["type"]
        before += len(t) > 1 and t[0] == LB.S2 and (t == LB.S1).any()
    assert jumps >= 2 and single >= 3 and before >= 3


def test_gap_exactly_at_the_threshold_splits():
    tab = LB._table([0, 1, 2, 3, 4], [1, 1, 2, 1, 1], [1.0, 2.0, 2.5, 5.0, 5.5], [60.0] * 5)
    assert LB.groups(tab, 1) == [(0, 0, 1), (1, 1, 1), (3, 4, 2)]
    assert LB.groups(tab, 3.0) == [(0, 1, 2), (3, 4, 2)]
    assert LB.groups(tab, 3.0000001) == [(0, 4, 4)]
    st = LB.analyse(tab, 3.0)["groups"]
    assert st["id"].tolist() == [1] and st["pairs_count"].tolist() == [1]      # the second group has no pair


def test_types_from_tags_equal_the_strings():
    n = 0
    for name, _, c in LC.golden_cases():
        if c is None:
            continue
        a = LB.types_from_strings(c["raw"], c["fin"], dict(zip(c["raw"].tolist(), c["strings"])))
        b = LB.types_from_tags(c["raw"], c["fin"], c["tags"], c["gap"])
        assert np.array_equal(a, b), name
        n += int((c["gap"] != 0).sum())
    assert n > 0


def test_file_bytes_and_round_trip(tmp_path):
    forms = set()
    for name, fx, c in list(LC.golden_cases()) + list(LC.random_cases()):
        if c is None or bool(fx["none"]):
            continue
        got = LB.from_curve(c["raw"], LC.types_of(c), c["sr"], c["bt"], c["bv"], 5.0)
        text = LB.labels_csv_text(got)
        assert text.encode("utf-8") == str(fx["text"]).encode("utf-8"), name
        forms.add("sections" if text.startswith("# Peak Labels\n") else ("plain" if text != LB.HEADER else "empty"))
        path = str(tmp_path / f"{name}_labels.csv")
        assert LB.write_labels(path, got) is True
        assert open(path, "rb").read() == str(fx["text"]).encode("utf-8"), name
        back = LB.read_labels(path)
        for k in ("type", "time", "bpm"):
            assert back[k].tobytes() == got["table"][k].tobytes(), (name, k)
        assert (back["pos"] == -1).all()
    assert forms == {"sections", "plain", "empty"}


def test_empty_and_pairless_forms(tmp_path):
    assert LB.labels_csv_text(None) == "Time (s),Average BPM,Peak Type\n"
    empty = LB.analyse(LB.empty_table())
    assert LB.labels_csv_text(empty) == LB.HEADER and empty["summary"]["avg_delta_t"] is None
    assert len(LB.parse_labels(LB.HEADER)["type"]) == 0
    assert len(LB.read_labels(str(tmp_path / "missing_labels.csv"))["type"]) == 0
    lone = LB.analyse(LB._table([0, 3], [1, 1], [0.5, 1.25], [80.0, 81.5]))
    assert LB.labels_csv_text(lone) == LB.HEADER + "0.5,80.0,S1\n1.25,81.5,S1\n"
    both = LB.analyse(LB._table([0, 1], [1, 2], [0.0005, 0.3015], [80.0, 80.0]))
    # the table keeps its values; only the intervals section goes through numpy's rounding
    assert LB.labels_csv_text(both) == ("# Peak Labels\n" + LB.HEADER + "0.0005,80.0,S1\n0.3015,80.0,S2\n"
                                        "\n# S1-S2 Intervals\nS1_Time,S2_Time,Delta_t,S1_BPM\n0.0,0.302,0.301,80.0\n")
    assert LB.parse_labels(LB.labels_csv_text(both))["time"].tolist() == [0.0005, 0.3015]


def test_an_existing_file_is_left_alone(tmp_path):
    path = LB.labels_path("/somewhere/rec one.wav", str(tmp_path))
    assert os.path.basename(path) == "rec one_labels.csv"
    hand = "Time (s),Average BPM,Peak Type\n1.0,70.0,S1\n"
    with open(path, "w") as f:
        f.write(hand)
    lab = LB.analyse(LB._table([0, 1], [1, 2], [0.5, 0.8], [80.0, 80.0]))
    assert LB.write_labels(path, lab) is False and open(path).read() == hand
    assert LB.write_labels(path, lab, overwrite=True) is True and open(path).read() == LB.labels_csv_text(lab)


@pytest.mark.parametrize("name", ["env_plateaus", "ref_44k_40s_clicks", "env_static_fallback", "ref_44k_short16"])
def test_from_analysis_on_the_host_route(name):
    g, params, hint, inp = TB.load_case(name)
    try:
        res = B.analyze_recording(inp["env"], inp["sr"], inp["floor"], inp["troughs"], inp["peaks"], params, hint)
    except KeyError as e:
        res = {"error": e}
    for gap in LC.GAPS:
        LC.assert_same(LB.from_analysis(res, inp["sr"], gap), LC.expected(LC.fixture(name), gap), (name, gap))
