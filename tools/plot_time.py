"""What the plot costs on the device route (needs the GPU).

    python tools/plot_time.py [--files 1024] [--secs 60] [--repeats 12] [--fig-files 6] [--out FILE]

Three measurements in one process, each alternating its versions after
warm-ups, as tools/packed_results.py does:

  kernel    device time of k_pack_plot (bpmx_profile events around the launch)
            for the metric batch, synthesised on the device and run once, at
            plot_downsample_factor 1 and 5
  download  bytes and host time of Detector.pack_plot + PlotSeries.to_host at
            both factors against Result.to_host, each ending in a stream
            synchronise
  figure    per file of a small batch of the same recordings, the device
            route (run_host_reports(plot=True) / files + build_figure_packed)
            against the only route to the same figure before it (run_host /
            files + analyze_recording + build_figure), at both factors; the
            two figures' plotly JSON must be equal.  plotly's write_html, which
            both routes then run, is timed beside them.

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FACTORS = (1, 5)


def _stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fig-files", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd import beats as B
    from bpm_analysis_amd import plot as PL
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("plot_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.run(pcm, fo, a.fs, params, mode=a.mode, d=d)
        tot, F = int(res.doff[-1]), a.files
        bufs = (torch.empty(tot, dtype=torch.float64, device=det.device),
                torch.empty(tot, dtype=torch.float64, device=det.device))
        st.synchronize()

        # ---- kernel ---------------------------------------------------------------------- #
        det.profile_only("k_pack_plot")
        kern = {k: [] for k in FACTORS}
        for rep in range(a.warmup + a.repeats):
            for k in FACTORS:
                det.profile(True)                      # clears the totals: one launch per reading
                ps = det.pack_plot(res, k, out=bufs)
                cnt, ms = det.profile_read()["k_pack_plot"]
                assert cnt == 1
                if rep >= a.warmup:
                    kern[k].append(ms)
        det.profile(False)
        det.profile_only("")
        kept = {k: int(sum(N.load().bpmx_plot_length(int(x), k) for x in np.diff(res.doff))) for k in FACTORS}

        # ---- download -------------------------------------------------------------------- #
        def full():
            r = res.to_host()
            st.synchronize()
            return r

        def series(k):
            def go():
                r = det.pack_plot(res, k).to_host()
                st.synchronize()
                return r
            return go

        versions = [("result_to_host", full)] + [(f"plot_series_k{k}", series(k)) for k in FACTORS]
        for _ in range(a.warmup):
            for _, fn in versions:
                fn()
        down = {k: [] for k, _ in versions}
        last = {}
        for _ in range(a.repeats):
            for k, fn in versions:
                t0 = time.perf_counter()
                last[k] = fn()
                down[k].append((time.perf_counter() - t0) * 1e3)
        for k in FACTORS:                              # same values, at the size timed
            for x, y in zip(last["result_to_host"], last[f"plot_series_k{k}"]):
                kf = y["plot_factor"]
                assert np.array_equal(x["env"][::kf], y["env_plot"], equal_nan=True)
                assert np.array_equal(x["floor"][::kf], y["floor_plot"], equal_nan=True)
        del last

    # ---- figure ---------------------------------------------------------------------------- #
    recs = []
    for f in range(a.fig_files):
        buf = np.empty(n, dtype=np.int16)
        N.load().bpmx_synth_host(1 + f, n, a.fs, 1, buf.ctypes.data)
        recs.append(buf)
    G = len(recs)
    fig = {}
    for k in FACTORS:
        p = dict(params, plot_downsample_factor=k)
        t = {key: [] for key in ("device_batch_per_file", "build_figure_packed", "parent_batch_per_file",
                                 "analyze_recording", "build_figure", "write_html")}
        for rep in range(a.warmup + a.repeats):
            keep = rep >= a.warmup
            t0 = time.perf_counter()
            new = det.run_host_reports(recs, a.fs, p, mode=a.mode, plot=True)
            t1 = time.perf_counter()
            old = det.run_host(recs, a.fs, p, mode=a.mode, resolve_ties=True)
            t2 = time.perf_counter()
            if keep:
                t["device_batch_per_file"].append((t1 - t0) * 1e3 / G)
                t["parent_batch_per_file"].append((t2 - t1) * 1e3 / G)
            for f in range(G):
                name = f"rec{f}.wav"
                t0 = time.perf_counter()
                fa = PL.build_figure_packed(name, p, new[f])
                t1 = time.perf_counter()
                r = old[f]
                ar = B.analyze_recording(r["env"], r["sr"], r["floor"], r["troughs"], r["peaks"], p, None)
                t2 = time.perf_counter()
                fb = PL.build_figure(name, p, r["sr"], np.asarray(r["env"], dtype=np.float64), ar["all_raw_peaks"],
                                     ar["analysis_data"], ar["final_metrics"])
                t3 = time.perf_counter()
                if keep:
                    t["build_figure_packed"].append((t1 - t0) * 1e3)
                    t["analyze_recording"].append((t2 - t1) * 1e3)
                    t["build_figure"].append((t3 - t2) * 1e3)
                if rep == 0:
                    assert fa.to_json() == fb.to_json(), (k, f)
                    with tempfile.TemporaryDirectory() as td:
                        t0 = time.perf_counter()
                        fa.write_html(os.path.join(td, "p.html"))
                        t["write_html"].append((time.perf_counter() - t0) * 1e3)
        s = {key: _stats(v) for key, v in t.items()}
        med = lambda key: s[key]["median_ms"]       # noqa: E731
        s["per_file_median_ms"] = {
            "device_route": round(med("device_batch_per_file") + med("build_figure_packed"), 3),
            "parent_route": round(med("parent_batch_per_file") + med("analyze_recording") + med("build_figure"), 3),
            "write_html_either_route": med("write_html")}
        fig[f"factor_{k}"] = s

    sm = 4 * F * 4
    obj = {
        "tool": "plot_time", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": F, "secs": a.secs, "fs": a.fs, "nd_per_file": int(res.doff[1]), "sum_nd": tot},
        "k_pack_plot_device_ms": {f"factor_{k}": dict(_stats(kern[k]), kept_entries=kept[k],
                                                      bytes_written=16 * kept[k],
                                                      written_GBps_at_median=round(
                                                          16 * kept[k] / statistics.median(kern[k]) / 1e6, 1))
                                  for k in FACTORS},
        "d2h_bytes": dict({"result_to_host": 4 * 8 * tot + sm}, **{f"plot_series_k{k}": 16 * kept[k] for k in FACTORS}),
        "to_host_ms": {k: _stats(v) for k, v in down.items()},
        "figure_per_file_ms": dict(fig, files=G),
    }
    line = json.dumps(obj)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
