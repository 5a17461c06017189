"""What the packed download saves on the metric batch (needs the GPU).

    python tools/packed_results.py [--files 1024] [--secs 60] [--repeats 12] [--out FILE]

The batch is synthesised on the device (Detector.synth).  Two versions of
"run, then bring the results to the host" alternate in one process, each
ending in a stream synchronise and timed by the host clock:

    full    Detector.run + Result.to_host      (env, floor, troughs, peaks as sum(Nd)-long arrays)
    packed  Detector.run + Detector.pack + Packed.to_host   (per-peak / per-trough tables)

and a third, informative only, adds the int16 debug samples to the packed one.
D2H bytes are computed from the array sizes (the packed ones from the totals
the run produced); the pack kernels' device time comes from bpmx_profile in a
run of its own after the timed ones.  Prints one JSON object."""
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
            "spread_ms": round(max(ms) - min(ms), 3), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--mode", default="native", choices=["native", "reference"])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd.design import design
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("packed_results.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    d = design(a.fs, params, log=False)
    n = int(a.secs * a.fs)
    fo = np.arange(a.files + 1, dtype=np.int64) * n
    st = det.host_stream()
    with torch.cuda.stream(st):
        pcm = det.synth(fo, a.fs, 1, seed0=1)
        res = det.alloc(fo, d.ds, d.sr)
        res_y = det.alloc(fo, d.ds, d.sr, want_y=True)
        pk = det.alloc_packed(res, d.distance)
        pk_y = det.alloc_packed(res_y, d.distance, want_y16=True)
        st.synchronize()

        def full():
            det.run(pcm, fo, a.fs, params, mode=a.mode, out=res, d=d)
            r = res.to_host()
            st.synchronize()
            return r

        def packed():
            det.run(pcm, fo, a.fs, params, mode=a.mode, out=res, d=d)
            r = det.pack(res, d.distance, out=pk).to_host()
            st.synchronize()
            return r

        def packed_y16():
            det.run(pcm, fo, a.fs, params, mode=a.mode, out=res_y, d=d)
            r = det.pack(res_y, d.distance, want_y16=True, out=pk_y).to_host()
            st.synchronize()
            return r

        versions = [("full", full), ("packed", packed), ("packed_y16", packed_y16)]
        for _ in range(a.warmup):
            for _, fn in versions:
                out = fn()
        times = {k: [] for k, _ in versions}
        for _ in range(a.repeats):                    # alternating, so drift and neighbours hit each alike
            for k, fn in versions:
                t0 = time.perf_counter()
                out = fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
                if k == "full":
                    f_res = out
                elif k == "packed":
                    p_res = out
        # same answers, at the size timed
        for x, y in zip(f_res, p_res):
            assert np.array_equal(x["peaks"], y["peaks"]) and np.array_equal(x["troughs"], y["troughs"])
            assert np.array_equal(x["env"][x["peaks"]], y["env_pk"], equal_nan=True)
            assert np.array_equal(x["floor"][x["peaks"]], y["floor_pk"], equal_nan=True)
        # device time of the pack kernels, in a run of its own
        det.profile(True)
        reps = 5
        for _ in range(reps):
            det.run(pcm, fo, a.fs, params, mode=a.mode, out=res_y, d=d)
            det.pack(res_y, d.distance, want_y16=True, out=pk_y)
        st.synchronize()
        prof = det.profile_read()
        det.profile(False)
    labels = ("k_pack_scan", "k_pack_gather", "k_y16_max", "k_y16_quant")
    kern = {k: round(prof[k][1] / prof[k][0], 4) for k in labels if k in prof}
    run_ms = sum(ms for k, (c, ms) in prof.items() if k not in labels) / reps
    F, tot = a.files, int(res.doff[-1])
    tp = sum(len(r["peaks"]) for r in p_res)
    tt = sum(len(r["troughs"]) for r in p_res)
    small_full = 4 * F * 4                              # n_troughs, n_peaks, n_raw_troughs, flags
    small_packed = 2 * (F + 1) * 8 + 2 * F * 4           # two offset arrays, n_raw_troughs, flags
    full_b = 4 * 8 * tot + small_full
    packed_b = tp * (4 + 8 + 8) + tt * (4 + 8) + small_packed
    fm, pm = _stats(times["full"]), _stats(times["packed"])
    gain = fm["median_ms"] - pm["median_ms"]
    spread = max(fm["spread_ms"], pm["spread_ms"])
    obj = {
        "tool": "packed_results", "device": torch.cuda.get_device_name(0), "mode": a.mode,
        "batch": {"files": F, "secs": a.secs, "fs": a.fs, "nd_per_file": int(res.doff[1]), "sum_nd": tot,
                  "raw_peaks": tp, "troughs": tt, "table_capacity": pk.cap_peaks},
        "d2h_bytes": {"full": full_b, "packed": packed_b, "packed_with_y16": packed_b + 2 * tot + 8 * F,
                      "full_with_y": full_b + 8 * tot, "ratio_full_over_packed": round(full_b / max(packed_b, 1), 1)},
        "pack_kernels_device_ms": dict(kern, tables_total=round(kern.get("k_pack_scan", 0) + kern.get("k_pack_gather", 0), 4),
                                       y16_total=round(kern.get("k_y16_max", 0) + kern.get("k_y16_quant", 0), 4)),
        "run_kernels_device_ms": round(run_ms, 3),
        "host_clock_ms": {"run_plus_to_host": fm, "run_plus_pack_plus_packed_to_host": pm,
                          "same_with_y16": _stats(times["packed_y16"]),
                          "per_repeat": {k: [round(v, 3) for v in ms] for k, ms in times.items()}},
        "verdict": {"median_gain_ms": round(gain, 3), "largest_spread_ms": spread,
                    "packed_wins_beyond_spread": bool(gain > spread),
                    "speedup_median": round(fm["median_ms"] / pm["median_ms"], 2)},
    }
    line = json.dumps(obj)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
