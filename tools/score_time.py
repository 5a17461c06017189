"""Scoring against corrected labels on the device against the host route, and
the settings sweep against one full host analysis per setting, on the metric
batch (needs the GPU).

    python tools/score_time.py [--files 1024] [--secs 60] [--repeats 12] [--settings 8] [--sweep-repeats 12]
                               [--out FILE.json]

The batch is synthesised on the device and run, packed and taken through the
traced beat stages and the labels stage once; the reference marks are the
labels of that run after the corrections a person could make (marks moved
within and beyond the tolerance, removed, renamed).  Every timed version then
starts from the same tables in HBM, in one process:

    kernel      Detector.score_device with the rows, HIP events around the launch (k_score alone)
    device_e2e  score_device(rows=False) + Scores.download: the integer records on the host
    host_e2e    Labels.to_host + labels.score per file: the route without the device stage
                (host_download: the Labels.to_host part of it)
    sweep_device  Detector.score_sweep over --settings settings: PCM up once, the envelope once,
                  one download of record[P, F, 20]
    sweep_host    run_host_reports(labels=True) + labels.score, once per setting

The versions alternate, so drift and neighbours hit each alike.  The records
of the routes are compared at the size timed.  Prints one JSON object and
writes it to --out (appending to the list a file already holds)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3),
            "n": len(ms)}


def _verdict(s, dev, host):
    dm, hm = s[dev]["median_ms"], s[host]["median_ms"]
    spread = max(s[dev]["max_ms"] - s[dev]["min_ms"], s[host]["max_ms"] - s[host]["min_ms"])
    won = "device" if hm - dm > spread else ("host" if dm - hm > spread else "neither (within the spread)")
    return {"difference_of_medians_ms": round(hm - dm, 3), "larger_spread_ms": round(spread, 3), "won": won}


def corrected(table, seed):
    """A person's corrections of a label table: a third of the marks moved by up to 40 ms, a tenth by 60 .. 150 ms,
    a tenth removed, a tenth renamed."""
    from bpm_analysis_amd import labels as LB
    if table is None:
        return LB.empty_table()
    rng = np.random.default_rng(seed)
    n = len(table["time"])
    u = rng.random(n)
    move = np.where(u < 0.33, rng.integers(-40, 41, n), np.where(u < 0.43, rng.integers(60, 151, n), 0)) / 1000.0
    typ = np.where(rng.random(n) < 0.1, 3 - table["type"], table["type"])
    keep = rng.random(n) >= 0.1
    return LB._table(table["pos"][keep], typ[keep], np.round(table["time"] + move, 3)[keep], table["bpm"][keep])


def settings(params, count):
    """`count` settings around the defaults that differ in the four keys a sweep usually turns."""
    out = []
    for k in range(count):
        out.append(dict(params, min_peak_distance_sec=(0.05, 0.1, 0.2, 0.15)[k % 4],
                        noise_floor_quantile=(0.2, 0.5, 0.35, 0.1)[(k // 2) % 4],
                        pairing_confidence_threshold=(0.5, 0.6)[(k // 4) % 2],
                        trough_rejection_multiplier=(4.0, 3.0, 5.0)[k % 3]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settings", type=int, default=8)
    ap.add_argument("--sweep-repeats", type=int, default=12, help="0: leave the sweep out")
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--gap", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import labels as LB
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("score_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        det.resolve_ties(res, params)
        beats = det.beats_device(det.pack(res, d.distance), params, trace=True)
        lab = det.labels_device(beats, a.gap)
        refs = [corrected(None if r is None else r["table"], 5 + f) for f, r in enumerate(lab.to_host())]
        marks = det.upload_marks(refs)
        st.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def kernel():
            ev0.record(st)
            det.score_device(lab, marks, a.tol, a.gap)
            ev1.record(st)
            st.synchronize()
            return ev0.elapsed_time(ev1)

        def device_e2e():
            t0 = time.perf_counter()
            r = det.score_device(lab, marks, a.tol, a.gap, rows=False).download()
            return (time.perf_counter() - t0) * 1e3, r[0]

        def host_e2e():
            t0 = time.perf_counter()
            rows = lab.to_host()
            st.synchronize()
            t1 = time.perf_counter()
            r = [LB.score(None if row is None else row["table"], m, a.tol, a.gap)["record"]
                 for row, m in zip(rows, marks.host)]
            t2 = time.perf_counter()
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, np.array(r)

        times = {k: [] for k in ("kernel", "device_e2e", "host_e2e", "host_download")}
        for it in range(a.warmup + a.repeats):
            kn = kernel()
            de = device_e2e()
            he = host_e2e()
            if it >= a.warmup:
                times["kernel"].append(kn)
                times["device_e2e"].append(de[0])
                times["host_e2e"].append(he[0])
                times["host_download"].append(he[1])
    same = de[1].tolist() == he[2].tolist()
    total = LB.score_total(de[1])
    s = {k: _stats(v) for k, v in times.items()}
    obj = {
        "tool": "score_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": a.files, "secs": a.secs, "fs": a.fs, "tol_sec": a.tol, "gap_sec": a.gap,
                  "labels": int(total[LB.SR_N_OUTSIDE] + total[LB.SR_N_DET] + total[LB.SR_PER_TYPE + LB.SR_N_DET]),
                  "reference_marks": int(marks.cap_ref), "total_record": total.tolist(),
                  "table_capacity": int(beats.packed.cap_peaks)},
        "k_score_hip_events_ms": s["kernel"],
        "device_route_ms": s["device_e2e"],
        "host_route_ms": s["host_e2e"],
        "host_route_download_ms": s["host_download"],
        "results_identical": bool(same),
        "verdict": _verdict(s, "device_e2e", "host_e2e"),
    }
    if a.sweep_repeats > 0:
        grid = settings(params, a.settings)
        host_pcm = pcm.cpu().numpy()
        recs = [host_pcm[f * n:(f + 1) * n] for f in range(a.files)]
        del pcm, res, beats, lab

        def sweep_device():
            t0 = time.perf_counter()
            r = det.score_sweep(recs, a.fs, grid, refs, mode=a.mode, tol_sec=a.tol, gap_sec=a.gap)
            return (time.perf_counter() - t0) * 1e3, r[0]

        def sweep_host():
            t0 = time.perf_counter()
            out = []
            for p in grid:
                rows = det.run_host_reports(recs, a.fs, p, mode=a.mode, labels=True, label_gap_sec=a.gap)
                out.append([LB.score(None if r.get("labels") is None else r["labels"]["table"], ref, a.tol,
                                     a.gap)["record"] for r, ref in zip(rows, refs)])
            return (time.perf_counter() - t0) * 1e3, np.array(out)

        sw = {"sweep_device": [], "sweep_host": []}
        warm = min(a.warmup, 1) if a.sweep_repeats < a.repeats else a.warmup
        for it in range(warm + a.sweep_repeats):
            sd = sweep_device()
            sh = sweep_host()
            if it >= warm:
                sw["sweep_device"].append(sd[0])
                sw["sweep_host"].append(sh[0])
        ss = {k: _stats(v) for k, v in sw.items()}
        obj["sweep"] = {"settings": a.settings, "warmup": warm, "device_ms": ss["sweep_device"],
                        "host_ms": ss["sweep_host"], "results_identical": bool(sd[1].tolist() == sh[1].tolist()),
                        "distinct_records": len({r.tobytes() for r in sd[1]}),
                        "verdict": _verdict(ss, "sweep_device", "sweep_host")}
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        runs = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                runs = json.load(fh)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(runs + [obj], indent=1) + "\n")


if __name__ == "__main__":
    main()
