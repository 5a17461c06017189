"""The shared, seeded cases of the marks tests (labels.rows_from_marks /
labels.revise, csrc/bpmx_marks_core.h as plain C++, k_marks on the GPU): mark
tables of 0 .. 700 marks, S1 counts at and beyond the LDS limit of marks_plan,
and the smallest shapes at which the stage can go wrong, at the rates 3, 147,
1000 and 44100.  Plus the file format of tests/marks_core_driver.cpp."""
import functools
import struct

import numpy as np

from bpm_analysis_amd import labels as LB
from bpm_analysis_amd.config import DEFAULT_PARAMS

WINDOW = float(DEFAULT_PARAMS["output_smoothing_window_sec"])
RATES = (3, 147, 1000, 44100)
COUNTS = (3, 63, 64, 65, 129, 700)
LIMIT = 624                      # S1 rows of marks_plan's LDS limit (test_marks_abi checks that it is)
I32_MAX = 2 ** 31 - 1
ND_EDGE = 5000


def _m(ms, typ, sr, nd=None, name=""):
    return {"name": name, "sr": int(sr), "nd": nd, "ms": np.asarray(ms, np.int64).astype(np.int32),
            "type": np.asarray(typ, np.int64).astype(np.int32)}


def generated(n, seed, sr):
    """n marks as a corrected file leaves them: ascending ms, S1 / S2 mostly alternating, some marks typed twice on
    one millisecond or one later (one row at a low rate), some of another type, one before the start."""
    rng = np.random.default_rng(seed)
    ms = np.cumsum(rng.integers(150, 600, n)).astype(np.int64)
    typ = np.where(np.arange(n) % 2 == 0, LB.S1, LB.S2)
    typ = np.where(rng.random(n) < 0.1, 3 - typ, typ)
    dup = np.flatnonzero(rng.random(n) < 0.06)
    dup = dup[dup > 0]
    ms[dup] = ms[dup - 1] + rng.integers(0, 2, len(dup))
    typ[dup] = 3 - typ[dup - 1]
    typ = np.where(rng.random(n) < 0.03, rng.choice([0, 3, -1], n), typ)
    if n > 2:
        ms[0] = -7
    order = np.argsort(ms, kind="stable")
    return ms[order], typ[order]


def all_s1(n, seed, sr=147):
    """n S1 marks on n different samples: n S1 rows."""
    rng = np.random.default_rng(seed)
    idx = np.cumsum(rng.integers(60, 160, n)).astype(np.int64)
    ms = (idx * 1000 + sr // 2) // sr                  # the millisecond nearest the sample
    return ms, np.full(n, LB.S1)


@functools.lru_cache(maxsize=1)
def cases():
    """[dict(name, sr, nd, ms, type)], seeded."""
    out = [
        _m([], [], 147, name="n0"),
        _m([1000], [1], 147, name="one_s1"),
        _m([1000], [2], 147, name="one_s2"),
        _m([500, 501], [1, 1], 1000, name="adjacent"),
        _m([1000, 1001], [1, 2], 147, name="same_sample"),
        _m([1000, 1001], [2, 1], 3, name="same_sample_s2_first"),
        _m([300, 900, 1500, 2200, 2900], [2] * 5, 147, name="only_s2"),
        _m([-5, -1, 0, 400, 900, 1300], [1, 2, 1, 2, 1, 2], 147, name="negative"),
        _m([1000, 1500, 2000, 48695490, 48695774, 48695775, 48700000, I32_MAX], [1, 2, 1, 1, 1, 1, 2, 1], 44100,
           name="int32_max"),
        _m([100, 600, 1100, ND_EDGE - 1, ND_EDGE, ND_EDGE + 1], [1, 2, 1, 1, 1, 2], 1000, nd=ND_EDGE, name="nd_edge"),
        _m([100, 600, 1100, 1700], [1, 2, 1, 1], 1000, nd=0, name="nd_zero"),
        _m([100, 200, 700, 800, 1300, 1400, 1900], [0, 3, 1, -1, 2, 1, 7], 147, name="other_types"),
        # beat times 2500, 2499 and 2501 ms apart: the centred 5 s window's closed right bound decides membership
        _m([0, 1000, 3500, 5999, 8500, 9500, 12000], [1] * 7, 1000, name="window_edges"),
    ]
    for k, n in enumerate(COUNTS):
        for j, sr in enumerate(RATES):
            if n in (3, 700) or (k + j) % 2 == 0:
                ms, typ = generated(n, 300 + 10 * k + j, sr)
                out.append(_m(ms, typ, sr, name=f"n{n}_sr{sr}"))
    for n in (LIMIT, LIMIT + 8):
        ms, typ = all_s1(n, 400 + n)
        out.append(_m(ms, typ, 147, name=f"s1_{n}"))
    ms, typ = all_s1(200, 77, 44100)
    out.append(_m(ms, typ, 44100, name="s1_200_sr44100"))
    return out


def params(window=WINDOW):
    return dict(DEFAULT_PARAMS, output_smoothing_window_sec=window)


def expect(case, window=WINDOW):
    """What the stage writes for one case, from labels.rows_from_marks and beats.bpm_series."""
    from bpm_analysis_amd import beats as B
    rows = LB.rows_from_marks(case, case["sr"], case["nd"])
    fin = rows["final"]
    w = {"idx": rows["idx"].astype(np.int32), "tag": rows["type"].astype(np.int8), "record": rows["record"],
         "status": LB.MARKS_OK if len(fin) >= 2 else LB.MARKS_FEW,
         "final": np.zeros(0, np.int32), "bpm_t": np.zeros(0), "bpm": np.zeros(0)}
    if len(fin) >= 2:
        s, t = B.bpm_series(fin, case["sr"], params(window))
        w["final"] = fin.astype(np.int32)
        if len(s):
            w["bpm_t"], w["bpm"] = np.asarray(t, np.float64), np.asarray(s.values, np.float64)
    return w


@functools.lru_cache(maxsize=1)
def expected():
    """expect() of every case, computed once and left unchanged."""
    return [expect(c) for c in cases()]


def check_identity(rec, n_marks):
    rec = np.asarray(rec).tolist()
    assert rec[LB.MK_N_ROWS] + rec[LB.MK_N_MERGED] + rec[LB.MK_N_DROPPED] + rec[LB.MK_N_OTHER] == n_marks
    assert rec[LB.MK_N_S1] + rec[LB.MK_N_S2] == rec[LB.MK_N_ROWS] and rec[6:] == [0, 0] and min(rec) >= 0


def assert_same(got, want, where):
    """Integers equal, doubles as bit patterns."""
    assert int(got["status"]) == int(want["status"]), where
    assert np.asarray(got["record"]).tolist() == np.asarray(want["record"]).tolist(), where
    for k in ("idx", "tag", "final"):
        assert np.asarray(got[k]).tolist() == np.asarray(want[k]).tolist(), (where, k)
    for k in ("bpm_t", "bpm"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (where, k)


# ---- the driver's files ------------------------------------------------------------------- #
def write_cases(path, window=WINDOW):
    """int32 n_cases; per case int32 nr, sr; int64 nd (-1: none); double window; int32 rf_ms[nr], rf_type[nr]."""
    with open(path, "wb") as f:
        cs = cases()
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<iiqd", len(c["ms"]), c["sr"], -1 if c["nd"] is None else c["nd"], window))
            f.write(c["ms"].tobytes() + c["type"].tobytes())


def read_results(path, n_cases):
    """Per case int32 status, record[8], n; int32 idx[n]; int8 tag[n]; int32 gap[n]; double env[n], floor[n];
    int32 n_final, final[n_final]; int32 n_bpm; double bpm_t[n_bpm], bpm[n_bpm]; double pass[3]."""
    raw = open(path, "rb").read()
    pos, out = 0, []

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(raw, dt, n, pos)
        pos += a.nbytes
        return a
    for _ in range(n_cases):
        r = {"status": int(take(np.int32, 1)[0]), "record": take(np.int32, LB.MARKS_RECORD)}
        n = int(take(np.int32, 1)[0])
        r["idx"], r["tag"], r["gap"] = take(np.int32, n), take(np.int8, n), take(np.int32, n)
        r["env"], r["floor"] = take(np.float64, n), take(np.float64, n)
        r["final"] = take(np.int32, int(take(np.int32, 1)[0]))
        m = int(take(np.int32, 1)[0])
        r["bpm_t"], r["bpm"], r["pass"] = take(np.float64, m), take(np.float64, m), take(np.float64, 3)
        out.append(r)
    assert pos == len(raw)
    return out
