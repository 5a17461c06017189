"""The labeler's output on the device against the host route, on the metric
batch (needs the GPU).

    python tools/labels_time.py [--files 1024] [--secs 60] [--repeats 12] [--gap 5.0] [--out FILE.json]

The batch is synthesised on the device and run, packed and taken through the
traced beat stages once; every timed version then starts from the same tables
in HBM, in one process:

    kernel      Detector.labels_device, HIP events around the launch (k_labels alone)
    device_e2e  labels_device + Labels.to_host: per-file labels dicts (table, pairs, groups, summary)
    host_e2e    Beats.to_host(explain=True) + labels.from_analysis per file: the route without the
                device stage, which needs the debug strings on the host to tell an S2
                (host_download: the Beats.to_host(explain=True) part of it)

The versions alternate, so drift and neighbours hit each alike.  The results
of the two routes are compared at the size timed.  Prints one JSON object and
writes it to --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gap", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import labels as LB
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("labels_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        beats = det.beats_device(det.pack(res, d.distance), params, trace=True)
        st.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def kernel():
            ev0.record(st)
            lab = det.labels_device(beats, a.gap)
            ev1.record(st)
            st.synchronize()
            return ev0.elapsed_time(ev1), lab

        def device_e2e():
            t0 = time.perf_counter()
            r = det.labels_device(beats, a.gap).to_host()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def host_e2e():
            t0 = time.perf_counter()
            rows = beats.to_host(explain=True)
            st.synchronize()
            t1 = time.perf_counter()
            r = [LB.from_analysis(row, d.sr, a.gap) for row in rows]
            t2 = time.perf_counter()
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, r

        times = {k: [] for k in ("kernel", "device_e2e", "host_e2e", "host_download")}
        for it in range(a.warmup + a.repeats):
            kn = kernel()
            de = device_e2e()
            he = host_e2e()
            if it >= a.warmup:
                times["kernel"].append(kn[0])
                times["device_e2e"].append(de[0])
                times["host_e2e"].append(he[0])
                times["host_download"].append(he[1])
    dev_res, host_res = de[1], he[2]
    same = all(LB.same(x, y) for x, y in zip(dev_res, host_res))
    have = [r for r in dev_res if r is not None]
    s = {k: _stats(v) for k, v in times.items()}
    dm, hm = s["device_e2e"]["median_ms"], s["host_e2e"]["median_ms"]
    spread = max(s["device_e2e"]["max_ms"] - s["device_e2e"]["min_ms"], s["host_e2e"]["max_ms"] - s["host_e2e"]["min_ms"])
    won = "device" if hm - dm > spread else ("host" if dm - hm > spread else "neither (within the spread)")
    obj = {
        "tool": "labels_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": a.files, "secs": a.secs, "fs": a.fs, "gap_sec": a.gap,
                  "files_with_labels": len(have), "labels": int(sum(r["summary"]["n_labels"] for r in have)),
                  "pairs": int(sum(r["summary"]["n_pairs"] for r in have)),
                  "groups_with_statistics": int(sum(len(r["groups"]["id"]) for r in have)),
                  "table_capacity": int(beats.packed.cap_peaks)},
        "k_labels_hip_events_ms": s["kernel"],
        "device_route_ms": s["device_e2e"],
        "host_route_ms": s["host_e2e"],
        "host_route_download_ms": s["host_download"],
        "results_identical": bool(same),
        "verdict": {"difference_of_medians_ms": round(hm - dm, 3), "larger_spread_ms": round(spread, 3), "won": won},
    }
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
