"""What packed 24-bit PCM costs in native mode against its int32 expansion
(needs the GPU).

    python tools/pcm24_time.py [--files 1024] [--secs 60] [--repeats 10] [--warmup 3] [--out profiles/pcm24.json]

One batch, 1024 x 60 s x 44.1 kHz mono at ds 146, with the PCM in HBM: the
synthetic int16 recordings times 256 plus a hashed low byte made on the
device, once as packed 3-byte samples and once expanded to the int32 array
scipy would make of the file.  Three routes alternate in one process after the
warm-ups, each on a context of its own (the block tables are cached per
context and keyed by the tile length, which differs between the routes), each
timed by HIP events around the whole step (every stage, as bench.py's step):

  i24      BPMX_DT_I24 on the matrix cores (k_native_blocks_mfma24)
  i32      the same samples as BPMX_DT_I32 (k_native_blocks_gen, f64 VALU)
  i24_f64  BPMX_DT_I24 with BPMX_OPT_NATIVE_F64 (k_native_blocks_gen)

and, in separate runs with bpmx_profile events on, the block kernel alone.
Medians and min-max; the block kernel's algorithmic traffic (the PCM once, 8
bytes per decimation block out) over its median time as bytes/s and as a share
of the MI355X's 8 TB/s.  The three routes' envelopes must agree within 1e-12 of
scale, i32 and i24_f64 bit for bit.  Prints one JSON object (and writes it to
--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BPS = 8.0e12


def _stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--fs", type=int, default=44100)
    ap.add_argument("--ds", type=int, default=146)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--routes", default="i24,i32,i24_f64",
                    help="which of them to run (i32 alone runs on a library built before the format existed)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from bpm_analysis_amd import DEFAULT_PARAMS
    from bpm_analysis_amd import _native as N
    from bpm_analysis_amd.engine import Detector, mode_design
    if not torch.cuda.is_available():
        sys.exit("pcm24_time.py measures on the GPU; none is visible")
    det = Detector(0)
    F, fs, n = a.files, a.fs, int(round(a.secs * a.fs))
    params = dict(DEFAULT_PARAMS, downsample_factor=a.ds, save_filtered_wav=False)
    d = mode_design(fs, params, "native")
    fo = np.arange(F + 1, dtype=np.int64) * n
    dev = det.device
    st = det.host_stream()
    with torch.cuda.stream(st):
        s16 = det.synth(fo, fs, 1, seed0=7)
        p24 = torch.empty(F * n * 3, dtype=torch.uint8, device=dev)
        x32 = torch.empty(F * n, dtype=torch.int32, device=dev)
        step = 64 * n
        for lo in range(0, F * n, step):                   # in pieces: the temporaries stay small
            hi = min(F * n, lo + step)
            i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            low = (((i * 2654435761) >> 13) & 255).to(torch.int32)
            v = s16[lo:hi].to(torch.int32)
            x32[lo:hi] = (v << 16) | (low << 8)
            b = p24[3 * lo:3 * hi].view(-1, 3)
            b[:, 0] = low.to(torch.uint8)
            b[:, 1] = (v & 255).to(torch.uint8)
            b[:, 2] = ((v >> 8) & 255).to(torch.uint8)
            del i, low, v
        del s16
        torch.cuda.empty_cache()
        routes = (("i24", p24, "i24", 0), ("i32", x32, None, 0), ("i24_f64", p24, "i24", N.OPT_NATIVE_F64))
        routes = tuple(r for r in routes if r[0] in a.routes.split(","))
        assert routes, "--routes names none of i24, i32, i24_f64"
        outs = {r: det.alloc(fo, d.ds, d.sr) for r, _, _, _ in routes}
        dets = {r: Detector(0) for r, _, _, _ in routes}

        def run(r, pcm, fmt, opt):
            dets[r].run(pcm, fo, fs, params, mode="native", out=outs[r], d=d, options=opt, sample_format=fmt)
        ms = {r: [] for r, _, _, _ in routes}
        for rep in range(a.warmup + a.repeats):
            for r, pcm, fmt, opt in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                run(r, pcm, fmt, opt)
                e1.record(st)
                e1.synchronize()
                if rep >= a.warmup:
                    ms[r].append(e0.elapsed_time(e1))
        kms = {r: [] for r, _, _, _ in routes}
        for x in dets.values():
            x.profile_only("k_native_blocks")
        for rep in range(1 + a.kernel_repeats):
            for r, pcm, fmt, opt in routes:
                dets[r].profile(True)                      # clears the totals: one run per reading
                run(r, pcm, fmt, opt)
                got = dets[r].profile_read()
                assert list(got) == ["k_native_blocks"] and got["k_native_blocks"][0] == 1, got
                if rep >= 1:
                    kms[r].append(got["k_native_blocks"][1])
        for x in dets.values():
            x.profile(False)
            x.profile_only("")
        st.synchronize()
        env = {r: outs[r].env for r in outs}
        err, same = None, None
        if len(env) == 3:
            scale = float(env["i32"].abs().max())
            err = float((env["i24"] - env["i32"]).abs().max()) / scale
            same = bool(torch.equal(env["i24_f64"].view(torch.int64), env["i32"].view(torch.int64)))
            assert same, "I24 with BPMX_OPT_NATIVE_F64 and I32 differ"
            assert err <= 1e-12, f"the matrix-core route is {err:.3e} of scale off the f64 kernel"
    nblocks = F * ((n + d.ds - 1) // d.ds - 1)
    res = {}
    for r, _, fmt, _ in routes:
        traffic = F * n * (3 if fmt else 4) + 8 * nblocks
        k = statistics.median(kms[r])
        res[r] = {"step": _stats(ms[r]), "block_kernel": dict(_stats(kms[r]), algorithmic_bytes=traffic,
                                                              bytes_per_s_at_median=round(traffic / (k * 1e-3), 0),
                                                              share_of_8TBps=round(traffic / (k * 1e-3) / PEAK_BPS, 4))}
    obj = {"tool": "pcm24_time", "device": torch.cuda.get_device_name(0), "library": "BPMX_LIB" if os.environ.get("BPMX_LIB") else "in-tree", "files": F,
           "frames_per_file": n, "fs": fs, "ds": d.ds, "repeats": a.repeats, "warmup": a.warmup, "routes": res,
           "env_i24_vs_i32_max_rel": err, "i24_f64_equals_i32": same}
    if "i24" in res and "i32" in res:
        obj["step_i32_minus_i24_ms_at_median"] = round(res["i32"]["step"]["median_ms"] - res["i24"]["step"]["median_ms"], 4)
    print(json.dumps(obj))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(obj, indent=1) + "\n")


if __name__ == "__main__":
    main()
