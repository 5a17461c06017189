"""The beat stages on the device against the host route, on the metric batch
(needs the GPU).

    python tools/beats_time.py [--files 1024] [--secs 60] [--repeats 12] [--threads 16] [--out FILE]

The batch is synthesised on the device and run and packed once; every timed
version then starts from the same packed tables in HBM, in one process:

    device      Detector.beats_device, HIP events around the launch (the stage alone)
    device_e2e  beats_device + Beats.to_host, host clock (what a caller waits for)
    host_e2e    Packed.to_host + _host.beats_batch on --threads threads, host clock
                (the route without the device stage: download, then host threads;
                the whole-array inputs beats_batch takes are prepared once, untimed)
    host_stage  _host.beats_batch alone over the downloaded tables

The versions alternate, so drift and neighbours hit each alike.  The results
of the two routes are compared at the size timed.  Prints one JSON object.
Under rocprofv3 the program goes after `--`."""
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


def _host_inputs(tabs):
    """beats_batch's per-file dicts from packed tables: env and floor as NaN
    arrays filled at the peaks (what _host.beats_packed builds per call)."""
    out = []
    for r in tabs:
        env, flo = np.full(r["n_env"], np.nan), np.full(r["n_env"], np.nan)
        env[r["peaks"]], flo[r["peaks"]] = r["env_pk"], r["floor_pk"]
        out.append(dict(env=env, floor=flo, peaks=r["peaks"], sr=r["sr"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _host as H
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("beats_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    bp = H.beat_params(params)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        pk = det.pack(res, d.distance)
        st.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def device():
            ev0.record(st)
            b = det.beats_device(pk, bp)
            ev1.record(st)
            st.synchronize()
            return ev0.elapsed_time(ev1), b

        def device_e2e():
            t0 = time.perf_counter()
            r = det.beats_device(pk, bp).to_host()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def host_e2e():
            t0 = time.perf_counter()
            tabs = pk.to_host()
            st.synchronize()
            t1 = time.perf_counter()
            r = H.beats_batch(inputs, bp, None, threads=a.threads)
            t2 = time.perf_counter()
            assert len(tabs) == len(inputs)
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, r

        tabs = pk.to_host()
        # built once, outside the timed region: every download brings the same tables, and the host
        # route's own O(n_peaks) scatter per file (_host.beats_packed) is left out in its favour
        inputs = _host_inputs(tabs)

        def host_stage():
            t0 = time.perf_counter()
            r = H.beats_batch(inputs, bp, None, threads=a.threads)
            return (time.perf_counter() - t0) * 1e3, r

        times = {k: [] for k in ("device", "device_e2e", "host_e2e", "host_download", "host_stage")}
        for it in range(a.warmup + a.repeats):
            dv = device()
            de = device_e2e()
            he = host_e2e()
            hs = host_stage()
            if it >= a.warmup:
                times["device"].append(dv[0])
                times["device_e2e"].append(de[0])
                times["host_e2e"].append(he[0])
                times["host_download"].append(he[1])
                times["host_stage"].append(hs[0])
        dev_res, host_res = de[1], he[2]
    same = True
    for x, y in zip(dev_res, host_res):
        if "error" in y:
            same &= "error" in x
            continue
        same &= bool(np.array_equal(x["final_peaks"], y["final_peaks"]) and np.array_equal(x["tags"], y["tags"]) and
                     np.array_equal(x["bpm"], y["bpm"], equal_nan=True) and
                     np.array_equal(x["bpm_times"], y["bpm_times"]))
    s = {k: _stats(v) for k, v in times.items()}
    obj = {
        "tool": "beats_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": a.files, "secs": a.secs, "fs": a.fs, "raw_peaks": int(sum(len(r["peaks"]) for r in tabs)),
                  "table_capacity": int(pk.cap_peaks), "host_threads": a.threads},
        "device_stage_hip_events_ms": s["device"],
        "device_route_ms": s["device_e2e"],
        "host_route_ms": s["host_e2e"],
        "host_route_download_ms": s["host_download"],
        "host_stage_alone_ms": s["host_stage"],
        "results_identical": bool(same),
        "verdict": {"device_route_not_slower": bool(s["device_e2e"]["median_ms"] <= s["host_e2e"]["median_ms"]),
                    "speedup_median": round(s["host_e2e"]["median_ms"] / max(s["device_e2e"]["median_ms"], 1e-9), 2)},
    }
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
