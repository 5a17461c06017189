"""The final metrics on the device against the host route, on the metric batch
(needs the GPU).

    python tools/metrics_time.py [--files 1024] [--secs 60] [--repeats 12] [--procs 16] [--out FILE]

The batch is synthesised on the device and run, packed and taken through the
beat stages once; every timed version then starts from the same beats and
curves in HBM, in one process:

    kernel      Detector.metrics_device, HIP events around the launch (k_metrics alone)
    download    metrics_device + Metrics.download: counts, records, HRV rows and runs on the host
    device_e2e  metrics_device + Metrics.to_host: per-file final_metrics dicts (what a caller reads)
    host_e2e    Beats.to_host + beats.final_metrics per file on --procs worker processes
                (the route without the device stage; the workers are started, and have imported
                pandas and scipy, before anything is timed; they never open the GPU)

The versions alternate, so drift and neighbours hit each alike.  The results
of the two routes are compared at the size timed.  Prints one JSON object and
writes a table to --out.  Under rocprofv3 the program goes after `--`."""
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


def _final_metrics(job):
    """Worker: beats.final_metrics of one file (None for fewer than two beats)."""
    from bpm_analysis_amd import beats as B
    peaks, sr, params = job
    if peaks is None or len(peaks) < 2:
        return None
    try:
        return B.final_metrics(peaks, sr, params)
    except ValueError as exc:
        return exc


def _same(a, b):
    """Two final_metrics dicts: summary, stats and table equal bit for bit."""
    if a is None or b is None or isinstance(b, Exception):
        return a is None and b is None
    ok = list(a["hrv_summary"]) == list(b["hrv_summary"])
    ok = ok and all(a["hrv_summary"][k] == v for k, v in b["hrv_summary"].items())
    for k in ("hrr_stats", "peak_recovery_stats", "peak_exertion_stats"):
        ok = ok and (a[k] is None) == (b[k] is None) and (a[k] is None or all(a[k][q] == v for q, v in b[k].items()))
    for k in ("major_inclines", "major_declines"):
        ok = ok and len(a[k]) == len(b[k]) and all(x == y for x, y in zip(a[k], b[k]))
    ha, hb = a["windowed_hrv_df"], b["windowed_hrv_df"]
    ok = ok and len(ha) == len(hb) and all(np.array_equal(ha[c].to_numpy(float), hb[c].to_numpy(float)) for c in ha)
    return bool(ok and a["smoothed_bpm"].equals(b["smoothed_bpm"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    # the workers first, from a process that has not touched the GPU, and by spawn: none of them opens it
    pool = multiprocessing.get_context("spawn").Pool(a.procs)
    from bpm_analysis_amd import DEFAULT_PARAMS
    pool.map(_final_metrics, [(np.arange(50, dtype=np.int64) * 300, 302, dict(DEFAULT_PARAMS))] * (4 * a.procs))
    import torch

    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("metrics_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    chunk = max(1, a.files // (4 * a.procs))
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        beats = det.beats_device(det.pack(res, d.distance), params)
        st.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def kernel():
            ev0.record(st)
            m = det.metrics_device(beats, params)
            ev1.record(st)
            st.synchronize()
            return ev0.elapsed_time(ev1), m

        def download():
            t0 = time.perf_counter()
            r = det.metrics_device(beats, params).download()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def device_e2e():
            t0 = time.perf_counter()
            r = det.metrics_device(beats, params).to_host()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def host_e2e():
            t0 = time.perf_counter()
            rows = beats.to_host()
            st.synchronize()
            t1 = time.perf_counter()
            jobs = [(r.get("final_peaks"), d.sr, params) for r in rows]
            r = pool.map(_final_metrics, jobs, chunksize=chunk)
            t2 = time.perf_counter()
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, r

        times = {k: [] for k in ("kernel", "download", "device_e2e", "host_e2e", "host_download")}
        for it in range(a.warmup + a.repeats):
            kn = kernel()
            dl = download()
            de = device_e2e()
            he = host_e2e()
            if it >= a.warmup:
                times["kernel"].append(kn[0])
                times["download"].append(dl[0])
                times["device_e2e"].append(de[0])
                times["host_e2e"].append(he[0])
                times["host_download"].append(he[1])
    pool.close()
    pool.join()
    dev_res, host_res, meta = de[1], he[2], dl[1][0]
    on_device = [r["metrics_source"] == "device" for r in dev_res]
    same = all(_same(x["final_metrics"], y) for x, y, dv in zip(dev_res, host_res, on_device) if dv)
    s = {k: _stats(v) for k, v in times.items()}
    dm, hm = s["device_e2e"]["median_ms"], s["host_e2e"]["median_ms"]
    spread = max(s["device_e2e"]["max_ms"] - s["device_e2e"]["min_ms"], s["host_e2e"]["max_ms"] - s["host_e2e"]["min_ms"])
    won = "device" if hm - dm > spread else ("host" if dm - hm > spread else "neither (within the spread)")
    obj = {
        "tool": "metrics_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": a.files, "secs": a.secs, "fs": a.fs, "final_beats": int(sum(len(r.get("final_peaks", ()))
                                                                                        for r in dev_res)),
                  "hrv_rows": int(meta["m_n_hrv"].sum()), "inclines": int(meta["m_n_inc"].sum()),
                  "declines": int(meta["m_n_dec"].sum()), "table_capacity": int(beats.packed.cap_peaks),
                  "worker_processes": a.procs,
                  "files_recomputed_on_host": int(len(on_device) - sum(on_device)),
                  "status_tie": int((meta["m_status"] == N.METRICS_TIE).sum())},
        "k_metrics_hip_events_ms": s["kernel"],
        "device_download_ms": s["download"],
        "device_route_ms": s["device_e2e"],
        "host_route_ms": s["host_e2e"],
        "host_route_download_ms": s["host_download"],
        "results_identical": bool(same),
        "verdict": {"difference_of_medians_ms": round(hm - dm, 3), "larger_spread_ms": round(spread, 3), "won": won},
    }
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        rows = [("k_metrics alone (HIP events)", "kernel"),
                ("device download  metrics_device + Metrics.download", "download"),
                ("device route     metrics_device + Metrics.to_host", "device_e2e"),
                (f"host route       Beats.to_host + final_metrics, {a.procs} processes", "host_e2e"),
                ("  of which the beats download (Beats.to_host)", "host_download")]
        with open(a.out, "w") as fh:
            fh.write(f"{'':62s}{'min':>9s}{'median':>9s}{'max':>9s}  (ms)\n")
            for label, k in rows:
                fh.write(f"{label:62s}{s[k]['min_ms']:9.3f}{s[k]['median_ms']:9.3f}{s[k]['max_ms']:9.3f}\n")
            fh.write("\n" + json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
