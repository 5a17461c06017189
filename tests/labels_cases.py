"""Cases shared by the label tests: the fixtures of tests/golden/labels (made
by the reference labeler's own functions, tests/golden/make_label_goldens.py),
their inputs from the beat goldens, the expected labels dicts, and the files of
tests/labels_core_driver.cpp."""
import functools
import os
import struct

import numpy as np

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import labels as LB
from tests import test_beats as TB

GOLD = os.path.join(TB.GOLD, "labels")
GAPS = (1, 3.0, 5.0)
TAG_OF = (("S1", 1), ("S2", 2), ("Lone S1", 3), ("Noise", 4))       # bpmx_beat_tag by the string's start
DEV_KEYS_I = ("lb_pos", "lb_type", "pr_s1", "pr_s2", "gr_id", "gr_first", "gr_last", "gr_s1", "gr_pairs")
DEV_KEYS_F = ("lb_time", "lb_bpm", "pr_dt", "gr_dt", "gr_bpm")


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: g[k] for k in g.files}


def tags_and_gap(strings):
    """(tags, gap) that give these final strings: the innermost string's type
    as the main pass' tag, each ORIGINAL_REASON wrapper as one gap-fill pass
    (the outermost the highest)."""
    tags, gap = np.zeros(len(strings), np.int8), np.zeros(len(strings), np.int32)
    for i, s in enumerate(strings):
        parts = str(s).split("§ORIGINAL_REASON§")
        base = parts[-1].strip()
        tags[i] = next((v for k, v in TAG_OF if base.startswith(k)), 0)
        wraps = parts[:-1]
        for j, w in enumerate(wraps):                 # outermost first
            it = len(wraps) - 1 - j
            gap[i] |= (N.TR_GAP_S2 if w.strip().startswith("S2") else N.TR_GAP_S1) << (2 * it)
    return tags, gap


@functools.lru_cache(maxsize=None)
def golden_cases():
    """[(name, fixture, case)]: a case is what the core and the kernel take."""
    out = []
    for name in TB.CASES:
        g = np.load(os.path.join(TB.GOLD, "beats", name + ".npz"))
        fx = fixture(name)
        if "final_peaks" not in g.files:
            out.append((name, fx, None))
            continue
        raw = g["all_raw_peaks"].astype(np.int64)
        info = dict(zip((int(k) for k in g["info_keys"]), (str(v) for v in g["info_vals"])))
        strings = [info.get(int(k), "") for k in raw]
        tags, gap = tags_and_gap(strings)
        has = "bpm_times" in g.files
        out.append((name, fx, dict(raw=raw, tags=tags, gap=gap, strings=strings, fin=g["final_peaks"].astype(np.int64),
                                   bt=g["bpm_times"] if has else np.zeros(0), bv=g["bpm_v"] if has else np.zeros(0),
                                   sr=int(g["sr"]), status=0)))
    return out


@functools.lru_cache(maxsize=None)
def random_cases():
    """[(name, fixture-like dict, case)] of _random.npz (sr = 1000)."""
    g = fixture("_random")
    out = []
    for c in range(int(g["n_cases"])):
        pre = f"c{c}_"
        fx = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
        fx["none"] = np.bool_(False)
        raw, types = fx["raw"].astype(np.int64), fx["types"]
        tags = np.where(types == 2, 2, np.where(types == 1, 1, 4)).astype(np.int8)
        gap = np.zeros(len(raw), np.int32)
        if c % 2:                                     # the same types through the gap labels over contrary tags
            sel = types == 2
            tags[sel] = 4
            gap[sel] = (N.TR_GAP_S1 << 2) | (N.TR_GAP_S2 << 6)
            sel = (types == 0) & (np.arange(len(raw)) % 2 == 0)
            tags[sel] = 2
            gap[sel] = N.TR_GAP_S2 | (N.TR_GAP_S1 << 4)
        out.append((f"random{c}", fx, dict(raw=raw, tags=tags, gap=gap, strings=None, fin=raw[types == 1],
                                           bt=fx["bt"], bv=fx["bv"], sr=1000, status=0, types=types)))
    return out


def types_of(case):
    if case.get("types") is not None:
        return case["types"]
    return LB.types_from_strings(case["raw"], case["fin"], dict(zip(case["raw"].tolist(), case["strings"])))


def host(case, gap_sec):
    """labels.py on a case; None where the stage makes no labels."""
    m = len(case["bt"])
    if case["status"] != 0 or len(case["fin"]) < 2 or m < 1 or m >= len(case["fin"]):
        return None
    return LB.from_curve(case["raw"], types_of(case), case["sr"], case["bt"], case["bv"], gap_sec)


def expected(fx, gap_sec):
    """The labels dict a fixture stands for (None: no labels)."""
    if bool(fx["none"]):
        return None
    t = fx["time"]
    row = lambda x: np.searchsorted(t, x).astype(np.int32)  # noqa: E731  (the times are unique and ascending)
    tag = f"g{gap_sec}_"
    n = len(fx["pair_dt"])
    tab = {"pos": fx["pos"].astype(np.int64), "type": fx["type"].astype(np.int8), "time": t.astype(np.float64),
           "bpm": fx["bpm"].astype(np.float64)}
    return {"table": tab,
            "pairs": {"s1": row(fx["pair_s1_time"]), "s2": row(fx["pair_s2_time"]), "dt": fx["pair_dt"]},
            "groups": {"id": fx[tag + "group_id"], "first": row(fx[tag + "start_time"]),
                       "last": row(fx[tag + "end_time"]), "s1_count": fx[tag + "s1_count"],
                       "pairs_count": fx[tag + "pairs_count"], "avg_delta_t": fx[tag + "avg_delta_t"],
                       "avg_bpm": fx[tag + "avg_bpm"]},
            "summary": {"n_labels": len(t), "n_s1": int((tab["type"] == 1).sum()), "n_s2": int((tab["type"] == 2).sum()),
                        "n_pairs": n, "avg_delta_t": float(fx["avg_delta_t"]) if n else None,
                        "avg_bpm": float(fx["avg_bpm"]) if n else None},
            "gap_sec": float(gap_sec)}


def assert_same(got, want, what=""):
    """Integers equal, doubles as bit patterns; says where they differ."""
    assert (got is None) == (want is None), what
    if want is None:
        return
    for part in ("table", "pairs", "groups"):
        assert list(got[part]) == list(want[part]), (what, part)
        for k in want[part]:
            a, b = np.asarray(got[part][k]), np.asarray(want[part][k])
            assert a.dtype == b.dtype and a.shape == b.shape, (what, part, k, a.dtype, b.dtype, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (what, part, k, a[:8], b[:8])
    assert LB.same(got, want), (what, got["summary"], want["summary"])


# ---- labels_core_driver's files ---------------------------------------------- #
def write_cases(path, cases, gap_sec):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<iiiiid", len(c["raw"]), len(c["fin"]), len(c["bt"]), c["sr"], c["status"],
                                float(gap_sec)))
            f.write(c["raw"].astype(np.int32).tobytes() + c["tags"].astype(np.int8).tobytes() +
                    c["gap"].astype(np.int32).tobytes() + c["fin"].astype(np.int32).tobytes() +
                    np.asarray(c["bt"], np.float64).tobytes() + np.asarray(c["bv"], np.float64).tobytes())


def read_results(path, n_cases):
    buf = open(path, "rb").read()
    o, out = 0, []
    for _ in range(n_cases):
        status, nl, npair, ng = struct.unpack_from("<iiii", buf, o)
        o += 16
        r = {"status": status, "record": np.frombuffer(buf, np.float64, N.LABELS_RECORD, o).copy()}
        o += 8 * N.LABELS_RECORD
        for k, dt, cnt in (("lb_pos", np.int32, nl), ("lb_type", np.int32, nl), ("lb_time", np.float64, nl),
                           ("lb_bpm", np.float64, nl), ("pr_s1", np.int32, npair), ("pr_s2", np.int32, npair),
                           ("pr_dt", np.float64, npair), ("gr_id", np.int32, ng), ("gr_first", np.int32, ng),
                           ("gr_last", np.int32, ng), ("gr_s1", np.int32, ng), ("gr_pairs", np.int32, ng),
                           ("gr_dt", np.float64, ng), ("gr_bpm", np.float64, ng)):
            r[k] = np.frombuffer(buf, dt, cnt, o).copy()
            o += cnt * np.dtype(dt).itemsize
        out.append(r)
    assert o == len(buf)
    return out


def labels_of(dev, gap_sec):
    """The labels dict of a driver / device result (None for BPMX_LABELS_NONE)."""
    if dev["status"] == N.LABELS_NONE:
        assert len(dev["lb_pos"]) == len(dev["pr_dt"]) == len(dev["gr_id"]) == 0 and np.isnan(dev["record"]).all()
        return None
    assert dev["status"] == N.LABELS_OK
    return LB.assemble(dev, gap_sec)
