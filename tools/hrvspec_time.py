"""Device time of the HRV spectrum (bpmx_hrvspec_device) by HIP events, both
forms of the kernel (needs the GPU).

    python tools/hrvspec_time.py [--repeats 15] [--warmup 3] [--out profiles/hrvspec_time.json]

Three batches of synthetic beats (a heart with respiratory and slow modulation,
uploaded once as corrected marks through ``Detector.marks_device``): 1024
recordings of 60 s at sr 302 and 64 of 540,000 samples at sr 300 at the stage's
defaults (120 s windows every 30 s, 256 frequencies), and the second again with
a window every 10 s.  Events bracket the two launches of one
``Detector.hrv_spectrum_device`` call on the detector's stream.  The two forms
(the rotation along the grid, and one sincos per term behind
BPMX_OPT_HRVSPEC_DIRECT) alternate call by call in one loop, so both see the
same machine; the median, minimum and maximum over --repeats calls after
--warmup are reported per form, with the term count of the definition (kept
intervals x frequencies, summed over the valid windows), the terms per second,
and the share of the f64 vector peak (78.6 TFLOPS) that the ten floating-point
operations of a term's six sums alone amount to: the sines and cosines are not
counted, so the share says how far the sums are from being the whole cost.
For context only, the file also records ``hrv_spectrum.spectrum`` (the numpy
statement) of one recording on one host thread, scaled to the batch.  Prints
one JSON object per batch and writes the list to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_PEAK_TFLOPS = 78.6
FLOPS_PER_TERM = 10          # two additions and four multiply-adds


def _stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def beats_ms(files, seconds, kinds=8):
    """`files` lists of beat times in ms over `seconds`: `kinds` distinct hearts, repeated."""
    base = []
    for k in range(kinds):
        rng = np.random.default_rng(100 + k)
        t, out, rr0 = 0.4, [], 60.0 / (58 + 9 * k)
        while t < seconds - 0.5:
            out.append(t)
            t += rr0 * (1 + 0.07 * np.sin(2 * np.pi * 0.25 * t + k) + 0.05 * np.sin(2 * np.pi * 0.09 * t)
                        + 0.01 * rng.standard_normal())
        base.append(np.round(np.array(out) * 1000.0).astype(np.int32))
    return [base[f % kinds] for f in range(files)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "hrvspec_time.json"))
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd import hrv_spectrum as HS
    from bpm_analysis_amd import labels as LB
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("hrvspec_time.py measures on the GPU; none is visible")
    det = Detector(0)
    st = det.host_stream()
    params = dict(DEFAULT_PARAMS)
    objs = []
    for files, n, sr, hop_sec in ((1024, 18124, 302, 30.0), (64, 540000, 300, 30.0), (64, 540000, 300, 10.0)):
        ms_lists = beats_ms(files, n / sr)
        tables = [dict(ms=m, type=np.full(len(m), LB.S1, np.int32)) for m in ms_lists]
        lengths = [n] * files
        g = HS.geometry(sr, params, hop_sec=hop_sec)
        times = {"rotate": [], "direct": []}
        with torch.cuda.stream(st):
            beats = det.marks_device(tables, sr, params, nd=lengths)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            got = {}
            for it in range(a.warmup + a.repeats):
                for form, opt in (("rotate", 0), ("direct", N.OPT_HRVSPEC_DIRECT)):
                    det.set_options(opt)
                    ev0.record(st)
                    hs = det.hrv_spectrum_device(beats, lengths=lengths, g=g)
                    ev1.record(st)
                    st.synchronize()
                    if it >= a.warmup:
                        times[form].append(ev0.elapsed_time(ev1))
                    got[form] = hs
            det.set_options(0)
            host = {k: v.to_host() for k, v in got.items()}
            fin = beats.to_host()[0]["final_peaks"]
            st.synchronize()
        t0 = time.perf_counter()
        want = HS.spectrum_ints(fin, n, sr, g)
        host_s = time.perf_counter() - t0
        for form in times:
            r = host[form][0]
            assert np.array_equal(r["code"], want["code"]) and np.array_equal(r["n_rr"], want["n_rr"]), form
            ok = want["code"] == 0
            assert np.allclose(r["lf"][ok], want["lf"][ok], rtol=1e-9) and np.allclose(r["hf"][ok], want["hf"][ok], rtol=1e-9)
        windows = int(got["rotate"].woff[-1])
        terms = sum(int(r["n_rr"][r["code"] == 0].sum()) for r in host["rotate"]) * g["n_freq"]
        obj = {"tool": "hrvspec_time", "device": torch.cuda.get_device_name(0),
               "batch": {"files": files, "samples": n, "sr": sr, "win": g["win"], "hop": g["hop"], "n_freq": g["n_freq"],
                         "windows": windows, "valid_windows": int(sum(r["record"][0] for r in host["rotate"]))},
               "terms": terms, "flops_per_term_counted": FLOPS_PER_TERM,
               "host_numpy_one_file_s": round(host_s, 4), "host_numpy_scaled_to_batch_s": round(host_s * files, 2)}
        for form, ms in times.items():
            s = _stats(ms)
            rate = terms / (s["median_ms"] * 1e-3)
            obj[form] = {"hrv_spectrum_device_hip_events_ms": s, "gterms_per_s_at_median": round(rate / 1e9, 2),
                         "fraction_of_f64_vector_peak": round(FLOPS_PER_TERM * rate / 1e12 / F64_PEAK_TFLOPS, 4)}
        print(json.dumps(obj), flush=True)
        objs.append(obj)
        del beats, got, hs
    det.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(objs, indent=1) + "\n")


if __name__ == "__main__":
    main()
