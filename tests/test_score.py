"""labels.score (detected marks scored against a person's corrected marks) on
hand-computed cases written out here, the identities of the record, the walk
against a brute-force maximum matching, the preparation of the reference marks
and the derived summary.  No GPU."""
import itertools

import numpy as np
import pytest

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import score_cases as SC

S1, S2 = LB.S1, LB.S2
TP, SWAP, FP, FN, OUT = LB.KIND_TP, LB.KIND_SWAP, LB.KIND_FP, LB.KIND_FN, LB.KIND_OUTSIDE


def tab(*marks):
    """A label table from (seconds, type) pairs."""
    return LB._table([-1] * len(marks), [m[1] for m in marks], [m[0] for m in marks], [60.0] * len(marks))


def rec(s1=(), s2=(), outside=0, spans=0):
    """A record from the nine fields per type (missing ones 0)."""
    r = np.zeros(LB.SCORE_RECORD, np.int64)
    r[:len(s1)] = s1
    r[LB.SR_PER_TYPE:LB.SR_PER_TYPE + len(s2)] = s2
    r[LB.SR_N_OUTSIDE], r[LB.SR_N_SPANS] = outside, spans
    return r.tolist()


#        name, detected, reference, tol, gap -> record, sc_kind, sc_ref, rf_kind, rf_det
CASES = [
    ("perfect", tab((1.0, S1), (1.3, S2), (2.0, S1), (2.3, S2)), tab((1.0, S1), (1.3, S2), (2.0, S1), (2.3, S2)), .05, 5.,
     rec((2, 2, 2), (2, 2, 2), spans=1), [TP] * 4, [0, 1, 2, 3], [TP] * 4, [0, 1, 2, 3]),
    ("swap", tab((1.0, S1), (1.3, S1), (2.0, S1)), tab((1.0, S1), (1.31, S2), (2.0, S1)), .05, 5.,
     rec((2, 3, 2, 1, 0, 0), (1, 0, 0, 0, 0, 0), spans=1), [TP, SWAP, TP], [0, 1, 2], [TP, SWAP, TP], [0, 1, 2]),
    # exactly tol away is a match with error -tol; tol + 1 away is an FP and an FN
    ("at_tol", tab((0.95, S1), (2.0, S2)), tab((1.0, S1), (2.051, S2)), .05, 5.,
     rec((1, 1, 1, 0, 0, 0, -50, 50, 50), (1, 1, 0, 0, 1, 1), spans=1), [TP, FP], [0, -1], [TP, FN], [0, -1]),
    # two detected marks within tol of one reference mark: the walk takes the first
    ("compete", tab((1.0, S1), (1.04, S1)), tab((1.02, S1),), .05, 5.,
     rec((1, 2, 1, 0, 1, 0, -20, 20, 20), spans=1), [TP, FP], [0, -1], [TP], [0]),
    # the second of two equal reference times is missed; the second of two equal detected times is false
    ("equal_ref", tab((1.0, S1),), tab((1.0, S1), (1.0, S1)), .05, 5.,
     rec((2, 1, 1, 0, 0, 1), spans=1), [TP], [0], [TP, FN], [0, -1]),
    ("equal_det", tab((1.0, S2), (1.0, S2)), tab((1.01, S2),), .05, 5.,
     rec((), (1, 2, 1, 0, 1, 0, -10, 10, 10), spans=1), [TP, FP], [0, -1], [TP], [0]),
    # 0.949 is one ms before the span [0.95, 2.05]; 2.05 is its last ms
    ("outside", tab((0.949, S1), (1.0, S1), (2.05, S2), (2.051, S2), (30.0, S1)), tab((1.0, S1), (2.0, S2)), .05, 5.,
     rec((1, 1, 1), (1, 1, 1, 0, 0, 0, 50, 50, 50), outside=3, spans=1), [OUT, TP, TP, OUT, OUT], [-1, 0, 1, -1, -1],
     [TP, TP], [1, 2]),
    # a step of exactly gap starts a new span, so 3.5 lies between two spans; gap - 1 does not, so it is false
    ("gap_exact", tab((1.0, S1), (3.5, S1), (6.0, S1)), tab((1.0, S1), (6.0, S1)), .05, 5.,
     rec((2, 2, 2), outside=1, spans=2), [TP, OUT, TP], [0, -1, 1], [TP, TP], [0, 2]),
    ("gap_less_1", tab((1.0, S1), (3.5, S1), (5.999, S1)), tab((1.0, S1), (5.999, S1)), .05, 5.,
     rec((2, 3, 2, 0, 1, 0), spans=1), [TP, FP, TP], [0, -1, 1], [TP, TP], [0, 2]),
    ("no_det", tab(), tab((1.0, S1), (1.3, S2)), .05, 5., rec((1, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 1), spans=1),
     [], [], [FN, FN], [-1, -1]),
    # rows of another type and without a time are dropped before anything else; the file need not be in order
    ("dropped", tab((1.0, S1), (1.3, S2)), tab((1.3, S2), (1.1, 0), (float("nan"), S1), (1.2, 3), (1.0, S1)), .05, 5.,
     rec((1, 1, 1), (1, 1, 1), spans=1), [TP, TP], [0, 1], [TP, TP], [0, 1]),
    # tol 0, gap 1 ms: only equal milliseconds match and every reference mark is a span of its own, so 3.0 is
    # outside; an S2 on an S1 is a swap, not a match
    ("tol_zero", tab((1.0, S1), (2.0, S2), (3.0, S1)), tab((1.0, S1), (2.0, S1), (3.001, S1)), 0., .001,
     rec((3, 1, 1, 0, 0, 1), (0, 1, 0, 1, 0, 0), outside=1, spans=3), [TP, SWAP, OUT], [0, 1, -1], [TP, SWAP, FN],
     [0, 1, -1]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed(case):
    name, det, ref, tol, gap, record, sc_kind, sc_ref, rf_kind, rf_det = case
    got = LB.score(det, ref, tol, gap)
    assert got["status"] == LB.SCORE_OK
    assert got["record"].tolist() == record
    assert (got["sc_kind"].tolist(), got["sc_ref"].tolist()) == (sc_kind, sc_ref)
    assert (got["rf_kind"].tolist(), got["rf_det"].tolist()) == (rf_kind, rf_det)
    assert got["record"].dtype == np.int64 and got["sc_kind"].dtype == np.int32
    SC.check_identities(got["record"], len(det["time"]))


def test_empty_sides_and_status():
    ref = tab((1.0, S1), (1.3, S2))
    none = LB.score(tab((1.0, S1), (9.0, S2)), LB.empty_table())
    assert none["status"] == LB.SCORE_NONE == N.SCORE_NONE and len(none["sc_kind"]) == len(none["rf_kind"]) == 0
    assert none["record"].tolist() == rec(outside=2)
    assert LB.score(tab((1.0, S1)), None)["status"] == LB.SCORE_NONE
    # the analysis made no labels: the reference marks still count as misses
    no = LB.score(None, ref)
    assert no["status"] == LB.SCORE_NO_LABELS == N.SCORE_NO_LABELS
    assert no["record"].tolist() == rec((1, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 1), spans=1)
    assert no["rf_kind"].tolist() == [FN, FN] and len(no["sc_kind"]) == 0
    assert LB.score(None, LB.empty_table())["status"] == LB.SCORE_NONE
    only_other = LB.score(tab((1.0, S1)), tab((1.0, 0), (2.0, 7)))
    assert only_other["status"] == LB.SCORE_NONE and only_other["marks"]["dropped"] == 2


def test_parameters_are_checked():
    t = tab((1.0, S1))
    for tol, gap in ((-0.001, 5.0), (0.05, 0.1), (0.05, 0.05), (2.5, 5.0)):
        with pytest.raises(ValueError, match="gap_ms > 2 \\* tol_ms"):
            LB.score(t, t, tol, gap)
    assert LB.score_ms(0.05, 5.0) == (50, 5000) and LB.score_ms(0.0, 0.001) == (0, 1)
    assert LB.score(t, t, 0.05, 0.101)["record"][LB.SR_TP] == 1


def test_identities_on_the_shared_cases():
    seen = set()
    for (name, det, _), want in zip(SC.cases(), SC.expected()):
        n = 0 if det is None else len(det["time"])
        SC.check_identities(want["record"], n)
        if want["status"] >= 0:
            assert len(want["sc_kind"]) == n and len(want["rf_kind"]) == len(want["marks"]["ms"]), name
            for j, (k, i) in enumerate(zip(want["sc_kind"].tolist(), want["sc_ref"].tolist())):
                assert (i >= 0) == (k in (TP, SWAP)), name
                if i >= 0:                            # partners point at each other and lie within the tolerance
                    assert want["rf_det"][i] == j and want["rf_kind"][i] == k, name
                    assert abs(int(want["det_ms"][j]) - int(want["marks"]["ms"][i])) <= SC.TOL_MS, name
                    same = int(det["type"][j]) == int(want["marks"]["type"][i])
                    assert same == (k == TP), name
        seen.add(int(want["status"]))
    assert seen == {LB.SCORE_OK, LB.SCORE_NO_LABELS, LB.SCORE_NONE}
    by = {n: w["record"] for (n, _, _), w in zip(SC.cases(), SC.expected())}
    assert by["n700"][LB.SR_SWAP] > 5 and by["n700"][LB.SR_N_OUTSIDE] > 5 and by["n700"][LB.SR_N_SPANS] >= 2
    assert by["n700"][LB.SR_MAX_ABS] == SC.TOL_MS and by["few_ref"][LB.SR_N_OUTSIDE] > 600


def _max_matching(D, R, tol):
    """The size of a maximum matching of |d - r| <= tol, by trying every assignment."""
    best = 0

    def go(j, used, size):
        nonlocal best
        if size + (len(D) - j) <= best:
            return
        if j == len(D):
            best = size
            return
        for i in range(len(R)):
            if not used >> i & 1 and abs(D[j] - R[i]) <= tol:
                go(j + 1, used | 1 << i, size + 1)
        go(j + 1, used, size)

    go(0, 0, 0)
    return best


def test_walk_is_a_maximum_matching():
    """The TP count of each type equals a brute-force maximum matching: 20 000 seeded cases of at most 8 marks
    per side, in one span (the gap is longer than the cases) so every detected mark takes part."""
    rng = np.random.default_rng(2024)
    n_cases = tight = 0
    for _ in range(20000):
        tol = int(rng.integers(0, 40))
        nd, nr = int(rng.integers(0, 9)), int(rng.integers(1, 9))
        d = np.sort(rng.integers(0, 200, nd))
        r = np.sort(rng.integers(0, 200, nr))
        dt, rt = rng.integers(1, 3, nd), rng.integers(1, 3, nr)
        got = LB.score(LB._table([-1] * nd, dt, d / 1000.0, np.zeros(nd)),
                       LB._table([-1] * nr, rt, r / 1000.0, np.zeros(nr)), tol / 1000.0, 1.0)
        inside = (d >= r[0] - tol) & (d <= r[-1] + tol)
        for k, typ in enumerate((S1, S2)):
            want = _max_matching(d[inside & (dt == typ)].tolist(), r[rt == typ].tolist(), tol)
            assert got["record"][k * LB.SR_PER_TYPE + LB.SR_TP] == want, (d, dt, r, rt, tol)
            tight += 0 < want < min((inside & (dt == typ)).sum(), (rt == typ).sum())
        assert got["record"][LB.SR_N_OUTSIDE] == (~inside).sum()
        n_cases += 1
    assert n_cases >= 20000 and tight > 2000


def test_walk_alone_against_brute_force():
    for D, R, tol in itertools.product([(0, 10, 20), (5, 5, 6), (0, 100)], [(9, 11, 30), (5,), (50, 60, 99, 101)],
                                       (0, 1, 10, 50)):
        pairs = LB._walk([(d, j) for j, d in enumerate(D)], [(r, i) for i, r in enumerate(R)], tol)
        assert len(pairs) == _max_matching(list(D), list(R), tol)
        assert all(abs(D[j] - R[i]) <= tol for j, i in pairs)


def test_marks_round_trip_through_the_label_file():
    """marks_from_table(read_labels(labels_csv_text(x))) gives x's marks back, whichever file format is written."""
    for name, det, _ in SC.cases():
        if det is None or len(det["time"]) == 0:
            continue
        for lab in (LB.analyse(det), {"table": det, "pairs": {"dt": np.zeros(0)}}):
            back = LB.marks_from_table(LB.parse_labels(LB.labels_csv_text(lab)))
            want = LB.marks_from_table(det)
            assert back["ms"].tolist() == want["ms"].tolist() and back["type"].tolist() == want["type"].tolist(), name
            assert back["dropped"] == 0 and back["ms"].dtype == np.int32 and back["type"].dtype == np.int32
            assert back["ms"].tolist() == np.rint(det["time"] * 1000.0).astype(np.int64).tolist()


def test_marks_are_sorted_stably_and_counted():
    m = LB.marks_from_table(tab((2.0, S1), (1.0, S2), (2.0, S2), (1.0004, S1), (float("nan"), S2), (0.5, 0)))
    assert m["ms"].tolist() == [1000, 1000, 2000, 2000] and m["type"].tolist() == [S2, S1, S1, S2]
    assert m["row"].tolist() == [1, 3, 0, 2] and m["dropped"] == 2
    assert LB.marks_from_table(None)["ms"].shape == (0,)
    assert LB.marks_from_table(tab((0.0005, S1), (0.0015, S1), (0.0025, S1)))["ms"].tolist() == [0, 2, 2]   # to even


def test_a_table_against_itself_is_all_tp():
    for name, det, _ in SC.cases():
        if det is None or len(det["time"]) == 0:
            continue
        got = LB.score(det, det, SC.TOL_SEC, SC.GAP_SEC)
        n1, n2 = int((det["type"] == S1).sum()), int((det["type"] == S2).sum())
        assert got["record"][:LB.SR_PER_TYPE].tolist() == [n1, n1, n1, 0, 0, 0, 0, 0, 0], name
        assert got["record"][LB.SR_PER_TYPE:18].tolist() == [n2, n2, n2, 0, 0, 0, 0, 0, 0], name
        assert got["record"][LB.SR_N_OUTSIDE] == 0 and set(got["sc_kind"].tolist()) == {TP}
        assert got["sc_ref"].tolist() == list(range(len(det["time"]))) == got["rf_det"].tolist()


def test_summary_and_totals():
    r = np.array(rec((10, 8, 6, 1, 1, 2, -30, 90, 40), (4, 5, 3, 2, 0, 0, 12, 12, 9), outside=3, spans=2), np.int64)
    s = LB.score_summary(r)
    assert s["S1"]["precision"] == 6 / 8 and s["S1"]["recall"] == 6 / 10
    assert s["S1"]["f1"] == pytest.approx(2 * 0.75 * 0.6 / 1.35)
    assert (s["S1"]["mean_err_sec"], s["S1"]["mean_abs_err_sec"], s["S1"]["max_abs_err_sec"]) == (-0.005, 0.015, 0.04)
    assert s["all"]["tp"] == 9 and s["all"]["n_ref"] == 14 and s["all"]["max_abs_err_sec"] == 0.04
    assert s["n_outside"] == 3 and s["n_spans"] == 2
    z = LB.score_summary(np.zeros(LB.SCORE_RECORD, np.int64))
    assert all(np.isnan(z["S2"][k]) for k in ("precision", "recall", "f1", "mean_err_sec", "max_abs_err_sec"))
    tot = LB.score_total([r, r])
    assert tot[LB.SR_TP] == 12 and tot[LB.SR_MAX_ABS] == 40 and tot[LB.SR_PER_TYPE + LB.SR_MAX_ABS] == 9
    assert tot[LB.SR_SUM_ERR] == -60 and LB.score_total(np.zeros((0, LB.SCORE_RECORD))).tolist() == [0] * 20


def test_mistake_list_text():
    det = tab((1.0, S1), (1.3, S2), (2.0, S1), (2.3, S2))
    got = LB.score(det, tab((1.01, S1), (1.32, S1), (2.0, S1), (9.0, S2)))
    assert LB.score_csv_text(det, got) == ("Time (s),Peak Type,Kind,Partner Time (s)\n1.3,S2,SWAP,1.32\n"
                                           "2.3,S2,OUTSIDE,\n9.0,S2,FN,\n")
    assert LB.score_csv_text(det, LB.score(det, det)) == "Time (s),Peak Type,Kind,Partner Time (s)\n"
