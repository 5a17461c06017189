"""The shared, seeded cases of the scoring tests (labels.score,
csrc/bpmx_score_core.h as plain C++, k_score on the GPU): detected label
tables of 0 .. 700 marks and one count above the LDS budget of score_plan, and
reference tables made from them the way a person corrects marks: jitter within
and beyond the tolerance, deletions, insertions, type flips and a cut into two
to four labelled spans.  Plus the file format of tests/score_core_driver.cpp."""
import functools
import struct

import numpy as np

from bpm_analysis_amd import labels as LB

SR = 302
TOL_SEC, GAP_SEC = 0.05, 3.0
TOL_MS, GAP_MS = 50, 3000
COUNTS = (0, 1, 2, 63, 64, 65, 129, 700)
OVER = 900                       # marks per side beyond score_plan's LDS budget (test_score_abi checks that it is)
ROWS = ("sc_kind", "sc_ref", "rf_kind", "rf_det")


def detected(n, seed):
    """A label table as labels_device makes it: times round(idx / sr, 3), ascending, S1 / S2 mostly alternating."""
    rng = np.random.default_rng(seed)
    idx = np.cumsum(rng.integers(40, 200, n)).astype(np.int64)
    typ = np.where(np.arange(n) % 2 == 0, LB.S1, LB.S2)
    flip = rng.random(n) < 0.1
    typ = np.where(flip, 3 - typ, typ)
    time = [round(float(i) / SR, 3) for i in idx.tolist()]
    return LB._table(np.arange(n), typ, time, rng.uniform(50, 180, n).round(3))


def corrected(table, seed, spans=1):
    """A reference table from `table`: what a person's corrections could leave."""
    rng = np.random.default_rng(seed)
    ms = np.rint(table["time"] * 1000.0).astype(np.int64)
    typ = table["type"].astype(np.int64)
    n = len(ms)
    u = rng.random(n)
    jit = np.where(u < 0.45, rng.integers(-TOL_MS, TOL_MS + 1, n),            # still the same beat, the edges included
                   np.where(u < 0.6, rng.choice([-1, 1], n) * rng.integers(TOL_MS + 1, 3 * TOL_MS, n), 0))
    if n > 4:
        jit[1], jit[2] = TOL_MS, -(TOL_MS + 1)
    ms = ms + jit
    typ = np.where(rng.random(n) < 0.12, 3 - typ, typ)                       # the other name
    keep = rng.random(n) >= 0.1                                               # marks removed
    if spans > 1 and n > 8:                                                   # a cut: nothing labelled for a while
        lo, hi = int(ms.min()), int(ms.max())
        for c in np.linspace(lo, hi, spans + 1)[1:-1]:
            keep &= ~((ms > c - GAP_MS) & (ms < c + GAP_MS))
    ms, typ = ms[keep], typ[keep]
    if n:
        k = max(1, n // 12)                                                   # marks the analysis missed
        ms = np.concatenate([ms, rng.integers(int(ms.min(initial=0)) - 500, int(ms.max(initial=0)) + 9000, k)])
        typ = np.concatenate([typ, rng.integers(1, 3, k)])
    order = rng.permutation(len(ms))                                          # a file need not be in order
    other = np.zeros(2, np.int64)                                             # two rows of another type, one NaN time
    time = np.concatenate([ms[order] / 1000.0, [1.0, np.nan]])
    typ = np.concatenate([typ[order], other + [0, LB.S1]])
    return LB._table([-1] * len(typ), typ, time, np.full(len(typ), 60.0))


@functools.lru_cache(maxsize=1)
def cases():
    """[(name, detected table or None, reference table)], seeded."""
    out = []
    for k, n in enumerate(COUNTS + (OVER,)):
        det = detected(n, 100 + k)
        out.append((f"n{n}", det, corrected(det, 200 + k, spans=2 + k % 3)))
    d700 = out[len(COUNTS) - 1][1]
    out.append(("same", d700, LB._table(d700["pos"], d700["type"], d700["time"], d700["bpm"])))
    out.append(("no_ref", detected(65, 7), LB.empty_table()))
    out.append(("no_labels", None, corrected(detected(64, 8), 9)))
    out.append(("no_labels_no_ref", None, LB.empty_table()))
    out.append(("no_det", detected(0, 1), corrected(detected(129, 10), 11, spans=3)))
    out.append(("one_span", detected(129, 12), corrected(detected(129, 12), 13, spans=1)))
    few = detected(700, 14)
    out.append(("few_ref", few, corrected(detected(7, 15), 16)))
    return out


@functools.lru_cache(maxsize=1)
def expected():
    """labels.score of every case, computed once and left unchanged."""
    return [LB.score(det, ref, TOL_SEC, GAP_SEC) for _, det, ref in cases()]


def check_identities(rec, n_labels):
    a, b = rec[:LB.SR_PER_TYPE], rec[LB.SR_PER_TYPE:2 * LB.SR_PER_TYPE]
    for r, o in ((a, b), (b, a)):
        assert r[LB.SR_N_DET] == r[LB.SR_TP] + r[LB.SR_SWAP] + r[LB.SR_FP]
        assert r[LB.SR_N_REF] == r[LB.SR_TP] + o[LB.SR_SWAP] + r[LB.SR_FN]
        assert r[LB.SR_SUM_ABS] >= abs(r[LB.SR_SUM_ERR]) and r[LB.SR_MAX_ABS] * r[LB.SR_TP] >= r[LB.SR_SUM_ABS]
        assert all(v >= 0 for i, v in enumerate(r.tolist()) if i != LB.SR_SUM_ERR)
    assert rec[LB.SR_N_OUTSIDE] + a[LB.SR_N_DET] + b[LB.SR_N_DET] == n_labels


def assert_same(got, want, where):
    """Two score results: status, record and the four row arrays, integers compared for equality."""
    assert int(got["status"]) == int(want["status"]), where
    assert np.asarray(got["record"]).tolist() == np.asarray(want["record"]).tolist(), where
    for k in ROWS:
        if k in got and got[k] is not None:
            assert np.asarray(got[k]).tolist() == np.asarray(want[k]).tolist(), (where, k)


# ---- the driver's files ------------------------------------------------------------------- #
def write_cases(path, tol_ms=TOL_MS, gap_ms=GAP_MS):
    """int32 n_cases; per case int32 nd, nr, tol_ms, gap_ms, labelled; double lb_time[nd]; int32 lb_type[nd],
    rf_ms[nr], rf_type[nr]."""
    with open(path, "wb") as f:
        cs = cases()
        f.write(struct.pack("<i", len(cs)))
        for _, det, ref in cs:
            m = LB.marks_from_table(ref)
            t = np.zeros(0) if det is None else det["time"]
            ty = np.zeros(0, np.int32) if det is None else det["type"].astype(np.int32)
            f.write(struct.pack("<5i", len(t), len(m["ms"]), tol_ms, gap_ms, det is not None))
            f.write(np.asarray(t, np.float64).tobytes() + ty.tobytes())
            f.write(m["ms"].astype(np.int32).tobytes() + m["type"].astype(np.int32).tobytes())


def read_results(path, n_cases):
    """Per case int32 status, int64 record[20], int32 nd, nr (0, 0 where no rows were written), then the rows."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for _ in range(n_cases):
        status, = struct.unpack_from("<i", raw, pos)
        rec = np.frombuffer(raw, np.int64, LB.SCORE_RECORD, pos + 4)
        nd, nr = struct.unpack_from("<2i", raw, pos + 4 + 8 * LB.SCORE_RECORD)
        pos += 12 + 8 * LB.SCORE_RECORD
        r = {"status": status, "record": rec}
        for k, n in zip(ROWS, (nd, nd, nr, nr)):
            r[k] = np.frombuffer(raw, np.int32, n, pos)
            pos += 4 * n
        out.append(r)
    assert pos == len(raw)
    return out
