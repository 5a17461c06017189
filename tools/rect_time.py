"""What the rectified-mode envelope costs on the device (needs the GPU).

    python tools/rect_time.py [--repeats 12] [--warmup 2] [--out profiles/rect_envelope.json]

Two inputs, int16 mono, random samples made on the device from a seed:

  debug_wavs  1024 x 18,124 samples at fs 302 (w = 30): the metric batch's
              filtered debug WAVs
  cd_rate     64 x 2,646,000 samples at 44.1 kHz (w = 4410)

Per input, the device time of the ENVELOPE stage's kernels (bpmx_profile events
around every k_rect_* launch, summed per run) for the default route and for
BPMX_OPT_RECT_SEQ, alternating in one process after the warm-ups; min / median
/ max.  The two routes' envelopes must be equal at the size timed.  The
algorithmic traffic (2 B in + 8 B out per sample) over the median kernel time
is given as bytes/s and as a share of the MI355X's 8 TB/s.  For context only,
the pandas recipe on one host thread on part of the same data, scaled to the
batch.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BPS = 8.0e12
SHAPES = (("debug_wavs", 1024, 18124, 302), ("cd_rate", 64, 2646000, 44100))


def _stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pandas-files", type=int, default=2, help="recordings of each input the host recipe is timed on")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd.engine import Detector
    if not torch.cuda.is_available():
        sys.exit("rect_time.py measures on the GPU; none is visible")
    det = Detector(0)
    params = dict(DEFAULT_PARAMS, save_filtered_wav=False)
    routes = (("default", 0), ("rect_seq", N.OPT_RECT_SEQ))
    shapes = {}
    st = det.host_stream()
    for name, F, n, fs in SHAPES:
        w = fs // 10
        fo = np.arange(F + 1, dtype=np.int64) * n
        with torch.cuda.stream(st):
            gen = torch.Generator(device=det.device)
            gen.manual_seed(1234)
            pcm = torch.randint(-32768, 32768, (F * n,), dtype=torch.int16, device=det.device, generator=gen)
            outs = {r: det.alloc(fo, 1, fs, want_floor=False, want_troughs=False, want_peaks=False) for r, _ in routes}
            ms = {r: [] for r, _ in routes}
            kernels = {}
            for rep in range(a.warmup + a.repeats):
                for r, opt in routes:
                    det.profile(True)                  # clears the totals: one run per reading
                    det.run(pcm, fo, fs, params, mode="rectified", stages=N.STAGE_ENVELOPE, out=outs[r], options=opt)
                    got = {k: v for k, v in det.profile_read().items() if k.startswith("k_rect")}
                    assert got and all(c == 1 for c, _ in got.values()), got
                    kernels[r] = {k: round(v, 4) for k, (_, v) in got.items()}
                    if rep >= a.warmup:
                        ms[r].append(sum(v for _, v in got.values()))
            det.profile(False)
            st.synchronize()
            same = bool(torch.equal(outs["default"].env.view(torch.int64), outs["rect_seq"].env.view(torch.int64)))
            assert same, f"{name}: the two routes' envelopes differ"
            host = pcm[:a.pandas_files * n].cpu().numpy()
            env0 = outs["default"].env[:n].cpu().numpy()
        t0 = time.perf_counter()
        for f in range(a.pandas_files):
            e = pd.Series(np.abs(host[f * n:(f + 1) * n])).rolling(window=w, min_periods=1, center=True).mean()
            if f == 0:
                assert np.array_equal(e.to_numpy(), env0), f"{name}: device envelope differs from pandas"
        host_ms = (time.perf_counter() - t0) * 1e3 / a.pandas_files * F
        traffic = 10 * F * n
        s = {"files": F, "samples_per_file": n, "fs": fs, "window": w, "algorithmic_bytes": traffic,
             "routes_equal": same, "last_run_kernels_ms": kernels}
        for r, _ in routes:
            med = statistics.median(ms[r])
            s[r] = dict(_stats(ms[r]), bytes_per_s_at_median=round(traffic / (med * 1e-3), 0),
                        share_of_8TBps=round(traffic / (med * 1e-3) / PEAK_BPS, 4))
        # at the HBM rate the stage would take traffic / 8 TB/s: launch-bound when that is
        # below the few microseconds a launch costs
        s["time_at_8TBps_ms"] = round(traffic / PEAK_BPS * 1e3, 4)
        s["launch_bound"] = bool(s["time_at_8TBps_ms"] < 0.005)
        s["pandas_one_thread_ms_scaled_from_files"] = {"files_timed": a.pandas_files, "batch_ms": round(host_ms, 1)}
        shapes[name] = s
        del pcm, outs
        torch.cuda.empty_cache()
    obj = {"tool": "rect_time", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "shapes": shapes}
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
