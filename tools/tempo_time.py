"""Device time of the tempo stage (bpmx_tempo_device) by HIP events (needs the GPU).

    python tools/tempo_time.py [--repeats 15] [--warmup 3] [--out profiles/tempo_time.json]

Two batches of synthetic envelopes (smoothed noise with heart-rate pulses,
made on the host, uploaded once): 1024 x 18,124 samples at sr 302 (a minute
each) and 64 x 540,000 at sr 300 (half an hour each), at the stage's defaults.
Events bracket the two launches of one ``Detector.tempo_device`` call on the
detector's stream; the median over --repeats calls after --warmup is reported,
with the multiply-adds of the definition (windows x lags x win) and the rate
they imply against the f64 vector peak of the device (78.6 TFLOPS: two
operations per multiply-add).  Only one form of the kernel exists (f64 VALU),
so there is nothing to alternate with.  For context only, the file also records
``tempo.tempogram`` of one recording on one host thread, scaled to the batch.
Prints one JSON object per batch and writes the list to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_PEAK_TFLOPS = 78.6


def _stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def envelopes(files, n, sr, kinds=8, seed=3):
    """`files` envelopes of `n` samples: `kinds` distinct ones, repeated."""
    rng = np.random.default_rng(seed)
    base = []
    for k in range(kinds):
        period = int(60 * sr / (55 + 11 * k))
        w = max(3, sr // 30)
        x = np.convolve(rng.random(n + w - 1), np.ones(w) / w, mode="valid")
        base.append(0.2 * x + np.exp(-0.5 * (((np.arange(n) % period) - period / 2) / (0.08 * period)) ** 2))
    return [base[f % kinds] for f in range(files)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "tempo_time.json"))
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import tempo as TP
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("tempo_time.py measures on the GPU; none is visible")
    det = Detector(0)
    st = det.host_stream()
    objs = []
    for files, n, sr in ((1024, 18124, 302), (64, 540000, 300)):
        envs = envelopes(files, n, sr)
        win, hop, kmin, kmax = TP.geometry(sr)
        fo = np.arange(files + 1, dtype=np.int64) * n
        with torch.cuda.stream(st):
            res = det.alloc(fo, 1, sr)
            res.env.copy_(torch.from_numpy(np.concatenate(envs)).to(det.device))
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for it in range(a.warmup + a.repeats):
                ev0.record(st)
                tp = det.tempo_device(res)
                ev1.record(st)
                st.synchronize()
                if it >= a.warmup:
                    ms.append(ev0.elapsed_time(ev1))
            got = tp.to_host()
            st.synchronize()
        t0 = time.perf_counter()
        want = TP.tempogram(envs[0], sr)
        host_s = time.perf_counter() - t0
        assert np.array_equal(got[0]["lag"], want["lag"]) and np.abs(got[0]["rho"] - want["rho"]).max() <= 1e-9
        windows = int(tp.woff[-1])
        nlag = kmax - kmin + 3
        fma = windows * nlag * win
        s = _stats(ms)
        obj = {"tool": "tempo_time", "device": torch.cuda.get_device_name(0), "form": "valu",
               "batch": {"files": files, "samples": n, "sr": sr, "win": win, "hop": hop, "kmin": kmin, "kmax": kmax,
                         "windows": windows, "lags": nlag},
               "tempo_device_hip_events_ms": s, "multiply_adds": fma,
               "tflops_at_median": round(2 * fma / (s["median_ms"] * 1e-3) / 1e12, 3),
               "fraction_of_f64_vector_peak": round(2 * fma / (s["median_ms"] * 1e-3) / 1e12 / F64_PEAK_TFLOPS, 4),
               "host_one_thread_one_file_s": round(host_s, 4), "host_one_thread_scaled_to_batch_s": round(host_s * files, 2)}
        print(json.dumps(obj), flush=True)
        objs.append(obj)
        del res, tp
    det.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(objs, indent=1) + "\n")


if __name__ == "__main__":
    main()
