"""The analysis of a person's corrected marks on the device against the host
route, on the metric batch (needs the GPU).

    python tools/marks_time.py [--files 1,16,128,1024] [--secs 60] [--repeats 9] [--procs 16] [--out FILE.json]

The largest batch is synthesised on the device, run, packed and taken through
the traced beat stages and the labels stage once; the marks are the labels of
that run after the corrections a person could make (marks moved, removed,
renamed), as tools/score_time.py makes them.  Every size then takes the first
files of that batch, in one process:

    device  Detector.upload_marks, marks_device, metrics_device, labels_device, then the download of the
            records and tables (Metrics.download and Labels.to_host)
            (kernels: HIP events around the three launches of marks_device alone)
    host    labels.revise per file on --procs worker processes (started before the GPU is opened; they
            never touch it)

The routes alternate after the warm-ups, so drift and neighbours hit each
alike.  The label tables of the two routes are compared at the size timed.
Prints one JSON object per size and writes them to --out (appending to the
list a file already holds)."""
import argparse
import json
import multiprocessing
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


def _revise(job):
    from bpm_analysis_amd import labels as LB
    marks, sr, params, gap = job
    r = LB.revise(marks, sr, params, gap)
    return r["labels"], r["record"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default="1,16,128,1024")
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--gap", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sizes = sorted(int(x) for x in a.files.split(","))
    pool = multiprocessing.get_context("spawn").Pool(a.procs)      # before the GPU is opened; the workers never open it
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import labels as LB
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("marks_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(sizes[-1] + 1, dtype=np.int64) * n
    st = det.host_stream()
    objs = []
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        det.resolve_ties(res, params)
        beats = det.beats_device(det.pack(res, d.distance), params, trace=True)
        tabs = det.labels_device(beats, a.gap).to_host()
        all_marks = [LB.marks_from_table(corrected(None if r is None else r["table"], 5 + f)) for f, r in enumerate(tabs)]
        st.synchronize()
        del pcm, res, beats
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # every worker imports pandas with its first job: one job each (and some more) before anything is timed
        pool.map(_revise, [(all_marks[0], d.sr, params, a.gap)] * (8 * a.procs), chunksize=1)
        for F in sizes:
            host_marks = all_marks[:F]
            jobs = [(m, d.sr, params, a.gap) for m in host_marks]
            chunk = max(1, F // (4 * a.procs))

            def kernels():
                up = det.upload_marks(host_marks)
                ev0.record(st)
                det.marks_device(up, d.sr, params)
                ev1.record(st)
                st.synchronize()
                return ev0.elapsed_time(ev1)

            def device():
                t0 = time.perf_counter()
                b = det.marks_device(det.upload_marks(host_marks), d.sr, params)
                met, lab = det.metrics_device(b, params), det.labels_device(b, a.gap)
                meta, rows = met.download()
                labs = lab.to_host()
                st.synchronize()
                return (time.perf_counter() - t0) * 1e3, labs, meta

            def host():
                t0 = time.perf_counter()
                out = pool.map(_revise, jobs, chunksize=chunk)
                return (time.perf_counter() - t0) * 1e3, [o[0] for o in out]

            times = {k: [] for k in ("kernels", "device", "host")}
            for it in range(a.warmup + a.repeats):
                kn = kernels()
                de = device()
                ho = host()
                if it >= a.warmup:
                    times["kernels"].append(kn)
                    times["device"].append(de[0])
                    times["host"].append(ho[0])
            same = all(LB.same(x, y) for x, y in zip(de[1], ho[1]))
            s = {k: _stats(v) for k, v in times.items()}
            obj = {"tool": "marks_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
                   "batch": {"files": F, "secs": a.secs, "fs": a.fs, "sr": int(d.sr), "gap_sec": a.gap,
                             "marks": int(sum(len(m["ms"]) for m in host_marks)), "host_processes": a.procs},
                   "marks_device_hip_events_ms": s["kernels"], "device_route_ms": s["device"],
                   "host_route_ms": s["host"], "label_tables_identical": bool(same),
                   "metrics_statuses": sorted({int(v) for v in de[2]["m_status"]}),
                   "verdict": _verdict(s, "device", "host")}
            print(json.dumps(obj), flush=True)
            objs.append(obj)
    pool.close()
    pool.join()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        runs = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                runs = json.load(fh)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(runs + objs, indent=1) + "\n")


if __name__ == "__main__":
    main()
