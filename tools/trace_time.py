"""What the decision trace costs, on the metric batch (needs the GPU).

    python tools/trace_time.py [--files 1024] [--secs 60] [--repeats 12] [--report-files 16] [--out FILE]

The batch is synthesised on the device and run and packed once; every timed
version starts from the same packed tables in HBM, in one process, and the
versions alternate, so drift and neighbours hit each alike:

    k_beats         Detector.beats_device, HIP events around the launch
    k_beats_trace   Detector.beats_device(trace=True), HIP events
    to_host         beats_device + Beats.to_host, host clock
    to_host_trace   beats_device(trace=True) + Beats.to_host(explain=True), host clock
                    (download of the trace and explain.assemble for every file)
    explain_alone   explain.assemble over every file again, from the downloaded slices
    download bytes of both, from the used table prefixes

Then, per file on the host, over --report-files recordings of the same kind:

    packed_reports  explain.assemble + reports.write_reports_packed
    python_reports  beats.analyze_recording + write_bpm_csv + reports.write_reports

Prints one JSON object.  Under rocprofv3 the program goes after `--`."""
import argparse
import json
import os
import statistics
import sys
import tempfile
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
    ap.add_argument("--report-files", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd import beats as B
    from bpm_analysis_amd import explain as X
    from bpm_analysis_amd import reports as RP
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("trace_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    st = det.host_stream()
    with torch.cuda.stream(st):
        fo = np.arange(a.files + 1, dtype=np.int64) * n
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        pk = det.pack(res, d.distance)
        st.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def kernel(trace):
            ev0.record(st)
            det.beats_device(pk, params, trace=trace)
            ev1.record(st)
            st.synchronize()
            return ev0.elapsed_time(ev1)

        def e2e(trace):
            t0 = time.perf_counter()
            r = det.beats_device(pk, params, trace=trace).to_host(explain=trace)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        times = {k: [] for k in ("k_beats", "k_beats_trace", "to_host", "to_host_trace")}
        for it in range(a.warmup + a.repeats):
            # the launch behind the traced download follows ~0.4 s of host work on an idle GPU and measures
            # slower whichever kernel it is: the two kernels take that place in turn
            first = bool(it & 1)
            k0 = kernel(first)
            k1 = kernel(not first)
            row = ((k1, k0) if first else (k0, k1)) + (e2e(False), e2e(True))
            if it >= a.warmup:
                times["k_beats"].append(row[0])
                times["k_beats_trace"].append(row[1])
                times["to_host"].append(row[2][0])
                times["to_host_trace"].append(row[3][0])
        plain, traced = row[2][1], row[3][1]
        # the host share of to_host_trace: explain.assemble over every file again, from the downloaded slices
        t_explain = []
        for _ in range(3):
            t0 = time.perf_counter()
            for r in traced:
                if "trace" in r:
                    X.assemble(r["raw_peaks"], int(pk.sr), params, r["trace"])
            t_explain.append((time.perf_counter() - t0) * 1e3)
        same = all(("error" in x) == ("error" in y) and
                   ("error" in x or (np.array_equal(x["final_peaks"], y["final_peaks"]) and
                                     np.array_equal(x["tags"], y["tags"]) and
                                     x["bpm"].tobytes() == y["bpm"].tobytes())) for x, y in zip(plain, traced))
        tp = int(sum(len(r["raw_peaks"]) for r in plain))
        F = a.files
        small = (F + 1) * 8 + 4 * F * 4 + 3 * F * 8          # pk_off, flags, n_final, n_bpm, status, pass
        b_plain = small + tp * (4 + 4 + 8 + 8 + 1)            # pk_idx, final, bpm_t, bpm, tags
        b_trace = b_plain + F * 4 + tp * (8 * N.TR_NFIELDS + 4 + 4 + 8 + 8 + 8 + 4)

        # ---- per file on the host ------------------------------------------------
        R = a.report_files
        fo2 = np.arange(R + 1, dtype=np.int64) * n
        pcm2 = det.synth(fo2, a.fs, 1, seed0=1)
        res2 = det.run(pcm2, fo2, a.fs, params, mode=a.mode, d=d)
        pk2 = det.pack(res2, d.distance, want_tr_floor=True)
        b2 = det.beats_device(pk2, params, trace=True)
        whole = res2.to_host()
        got = det.metrics_device(b2, params).to_host(explain=True)
        tabs = pk2.to_host()
        st.synchronize()
    t_packed, t_python, identical = [], [], True
    with tempfile.TemporaryDirectory() as tmp:
        new, old = os.path.join(tmp, "new"), os.path.join(tmp, "old")
        os.mkdir(new)
        os.mkdir(old)
        for f in range(R):
            r = dict(tabs[f], **got[f])
            if "error" in r or r.get("final_metrics") is None:
                continue
            name = os.path.join(tmp, f"rec{f}.wav")
            tr = r["trace"]                               # the file's slices, as Beats.to_host(explain=True) keeps them
            t0 = time.perf_counter()
            r["analysis_data"] = X.assemble(r["peaks"], r["sr"], params, tr)
            RP.write_reports_packed(name, new, r, None)
            t1 = time.perf_counter()
            w = whole[f]
            ref = B.analyze_recording(w["env"], w["sr"], w["floor"], w["troughs"], w["peaks"], params, None)
            B.write_bpm_csv(os.path.join(old, f"rec{f}_bpm_plot.csv"), ref["final_metrics"])
            RP.write_reports(name, old, np.asarray(w["env"], dtype=np.float64), w["sr"], ref["all_raw_peaks"],
                             ref["analysis_data"], ref["final_metrics"], None)
            t2 = time.perf_counter()
            t_packed.append((t1 - t0) * 1e3)
            t_python.append((t2 - t1) * 1e3)
            for sfx in ("_bpm_plot.csv", "_Analysis_Summary.md", "_Debug_Log.md", "_Analysis_Settings.json"):
                x = open(os.path.join(new, f"rec{f}{sfx}"), encoding="utf-8").read().split("\n")
                y = open(os.path.join(old, f"rec{f}{sfx}"), encoding="utf-8").read().split("\n")
                if sfx.endswith(".md"):
                    x, y = x[:1] + x[2:], y[:1] + y[2:]          # the timestamp line
                identical &= x == y
    s = {k: _stats(v) for k, v in times.items()}
    obj = {
        "tool": "trace_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": a.files, "secs": a.secs, "fs": a.fs, "raw_peaks": tp, "table_capacity": int(pk.cap_peaks)},
        "k_beats_hip_events_ms": s["k_beats"], "k_beats_trace_hip_events_ms": s["k_beats_trace"],
        "to_host_ms": s["to_host"], "to_host_trace_explain_ms": s["to_host_trace"],
        "explain_alone_ms": _stats(t_explain),
        "download_bytes": {"to_host": b_plain, "to_host_trace": b_trace,
                           "trace_bytes_per_raw_peak": 8 * N.TR_NFIELDS + 36},
        "results_identical_with_trace": bool(same),
        "per_file_host": {"files": len(t_packed), "packed_reports_ms": _stats(t_packed) if t_packed else None,
                          "python_reports_ms": _stats(t_python) if t_python else None,
                          "report_files_identical": bool(identical)},
    }
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
