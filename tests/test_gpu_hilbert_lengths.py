"""Native mode's Hilbert transforms swept over decimated lengths Nd.

The host picks one of three device transforms from Nd's factorisation (the
fused in-LDS kernel k_hilbert_env, the four-step DFT of k_longfft.hip, rocFFT
chirp-z in k_bluestein.hip), and inside each the stage code depends on the
factorisation again.  tests/test_hilbert_plan.py enumerates those plan
branches without a GPU and keeps FUSED_ND / LONGFFT_ND a cover of them; here
every such length runs, as an int16 mono recording at 44,100 Hz
(ds = 146, window 30, 62-block tiles) of Nd * 146 - (i mod 3) samples.

Per recording:
* reference: the GPU's own decimated signal y (want_y), then
  rolling_mean(|scipy.signal.hilbert(y)|, sr // 10) on the host in double;
  max |env - ref| <= 1e-12 max |ref|, the project's bound between transform
  paths (test_fused_hilbert_matches_rocfft_and_oracle).  The PCM carries
  wide-band noise and the test first asserts that no bin of fft(y) is below
  1e-4 of the largest, so a wrong twiddle or table row at any frequency shows.
* selection: the profile shows the kernels of the transform SWEEP_PLAN (the
  plan driver's prediction) names, launch for launch.
* a second run without y is bit-identical in env, floor, troughs, peaks and
  flags; there k_hilbert_env makes yd itself (HilbArgs::fy), and k_native_yd is
  not launched when the whole batch is fused.
* floor, troughs, raw peaks, the raw-trough count and the flags equal the
  oracle's env-level functions on the GPU's own envelope bit for bit
  (qr_select inside k_hilbert_env at every `per`).

The largest error per stage form / row kind is recorded (record_property);
DESIGN.md's Hilbert section lists what an MI355X gave."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import goldens as G
from tests.test_gpu_params import _check, _same
from tests.test_hilbert_plan import BLUESTEIN_ND, FUSED_ND, GEOMETRY_ND, LONGFFT_ND, SWEEP_PLAN

FS, DS = 44100, 146
TOL = 1e-12
FLAT = 1e-4                       # smallest |fft(y)| bin over the largest, at least
# The smallest of some 15,000 bins is an extreme value: with this recipe about
# one recording in a hundred dips below FLAT.  Each batch's first seed is the
# first one, counting up from a round number, with which all its recordings
# keep a factor of two above FLAT (found on the CPU with the oracle's y).
FUSED_SEED0 = [900, 943, 983, 1020, 1060]


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


def _recording(seed, n):
    """The oracle's synthetic heart sounds at half scale plus uniform integer
    noise in +-8000: energy in every bin of the decimated band."""
    noise = np.random.default_rng(seed).integers(-8000, 8001, size=n)
    return (O.synth(seed, n, FS, 1) // 2 + noise).astype(np.int16)


def _oracle_answer(env, params, fs):
    """tests/test_gpu_params.py's _answer(env, p, sr_fs=fs), without its memo."""
    d = O.derive(fs, params)
    floor, tr, fl = O.noise_floor(env, d, params)
    pk, ptie = O.raw_peaks(env, floor, d, params, return_tie=True)
    raw = O.find_peaks(env, distance=d.distance, negate=True,
                       prominence=O.quantile(env, params["trough_prominence_quantile"]))
    return dict(env=env, floor=floor, troughs=tr, peaks=pk, n_raw=len(raw), flags=fl | (O.F_PEAK_TIE if ptie else 0))


def _blu_groups(nds):
    """k_bluestein.hip (bluestein_hilbert) groups its recordings by (packing, L):
    even Nd packed over M = Nd / 2 points, odd Nd over M = Nd; L the power of
    two >= 2 M - 1, or three quarters of it where that still holds 2 M - 1."""
    groups = {}
    for nd in nds:
        pack = nd % 2 == 0
        m = nd // 2 if pack else nd
        L = 1
        while L < 2 * m - 1:
            L <<= 1
        if (L >> 2) * 3 >= 2 * m - 1 and L >= 4:
            L = (L >> 2) * 3
        groups.setdefault((pack, L), []).append(nd)
    return groups


def _expected_launches(nds):
    """Launch counts per kernel label for a batch in this order: one
    k_hilbert_env per run of equal fused Nd, the four-step sequence once for
    all long-FFT recordings, one chirp-z sequence per (packing, L) group."""
    kind = [SWEEP_PLAN[nd].split(":")[0] for nd in nds]
    runs = sum(1 for i, nd in enumerate(nds) if kind[i] == "fused" and (i == 0 or nds[i - 1] != nd))
    want = {"k_hilbert_env": runs}
    lf = any(k == "longfft" for k in kind)
    want.update({"k_lf_tr": 4 * lf, "k_lf_rows[A]": 2 * lf, "k_lf_rows[B]": 2 * lf, "k_lf_mid": 1 * lf})
    ng = len(_blu_groups([nd for nd, k in zip(nds, kind) if k == "bluestein"]))
    want.update({"k_blu_pre": ng, "k_blu_mid": ng, "k_blu_post": ng, "k_blu_mul": 2 * ng})
    want["k_native_env"] = int(any(k != "fused" for k in kind))
    return want


def _profiled(det, recs, fs, params, **kw):
    det.profile_only("")
    det.profile(True)
    res = det.run_host(recs, fs, params, mode="native", longest_first=False, **kw)
    det.profile(False)
    return res, {k: v[0] for k, v in det.profile_read().items()}


def _sweep(det, record_property, nds, params=None, fs_ds=DS, seed0=900, fy=True, flat=FLAT):
    """Everything the module's docstring lists, for one ragged batch; returns
    (with_y results, references)."""
    import scipy.signal
    params = dict(G.BASE_PARAMS) if params is None else params
    d = O.derive(FS, params)
    assert d.ds == fs_ds
    recs = [_recording(seed0 + i, nd * d.ds - (i % 3)) for i, nd in enumerate(nds)]
    with_y, prof = _profiled(det, recs, FS, params, want_y=True)
    # the inputs, before any comparison
    refs = []
    for nd, r in zip(nds, with_y):
        y = np.ascontiguousarray(r["y"])
        assert y.size == nd == r["env"].size and r["sr"] == d.sr
        mag = np.abs(np.fft.fft(y))
        assert flat is None or mag.min() >= flat * mag.max(), (nd, mag.min() / mag.max())
        refs.append(O.rolling_mean(np.abs(scipy.signal.hilbert(y)), d.sr // 10, 1))
    # selection
    want = _expected_launches(nds)
    assert {k: prof.get(k, 0) for k in want} == want, (nds, prof)
    assert prof.get("k_native_yd", 0) == 1
    # the envelope
    worst = {}
    for nd, r, ref in zip(nds, with_y, refs):
        err = float(np.max(np.abs(r["env"] - ref)) / np.max(np.abs(ref)))
        worst[SWEEP_PLAN[nd]] = max(worst.get(SWEEP_PLAN[nd], 0.0), err)
        print(f"Nd={nd} {SWEEP_PLAN[nd]}: max|env - ref| / max|ref| = {err:.3e}")
    for label, err in sorted(worst.items()):
        record_property(f"max_rel_err[{label}]", err)
    for nd, r, ref in zip(nds, with_y, refs):
        assert np.max(np.abs(r["env"] - ref)) <= TOL * np.max(np.abs(ref)), (nd, SWEEP_PLAN[nd])
    # without y: k_hilbert_env builds yd of the fused recordings' full tiles itself
    plain, prof2 = _profiled(det, recs, FS, params)
    assert {k: prof2.get(k, 0) for k in want} == want, (nds, prof2)
    all_fused = all(SWEEP_PLAN[nd].startswith("fused") for nd in nds)
    if fy:                                                    # 62-block tiles: an even count, which fy needs
        assert prof2.get("k_native_yd", 0) == (0 if all_fused else 1)
    for nd, a, b in zip(nds, plain, with_y):
        for k in ("env", "floor", "troughs", "peaks"):
            assert _same(a[k], b[k]), (nd, k)
        assert a["flags"] == b["flags"] and a["n_raw_troughs"] == b["n_raw_troughs"], nd
    # detection on the GPU's own envelope
    for nd, r in zip(nds, plain):
        _check(r, _oracle_answer(np.ascontiguousarray(r["env"]), params, FS), (nd, SWEEP_PLAN[nd]))
    return with_y, refs


# Ragged batches of about 20 lengths.  Five hold fused lengths only (every
# fifth of FUSED_ND, so each mixes short and long recordings), two of them with
# a length twice in a row: one k_hilbert_env launch covers a run of equal Nd.
# The long-FFT lengths share one batch with a few fused lengths between them.
def _twice(nds, k):
    return nds[:k + 1] + nds[k:]


FUSED_BATCHES = [FUSED_ND[b::5] for b in range(5)]
FUSED_BATCHES[1] = _twice(FUSED_BATCHES[1], 3)
FUSED_BATCHES[4] = _twice(FUSED_BATCHES[4], 16)
LONGFFT_BATCH = LONGFFT_ND[:6] + [74] + _twice(LONGFFT_ND[6:12], 2) + [1024, 48] + LONGFFT_ND[12:]
# rocFFT chirp-z: odd Nd below 64, 2 x a prime beyond the four-step rows'
# reach, a large prime; with one fused and one long-FFT length between them.
# Few groups: creating a group's rocFFT plans takes most of a second.
BLUESTEIN_BATCH = BLUESTEIN_ND[:2] + [150] + BLUESTEIN_ND[2:4] + [247] + BLUESTEIN_ND[4:]
# one length per transform and form for the rocFFT R2C / C2R cross-check (a plan per length)
CROSS_BATCH = [18, 63, 150, 247, 12101]


def test_batches_hold_every_swept_length():
    assert sorted({nd for b in FUSED_BATCHES for nd in b}) == FUSED_ND
    assert all(SWEEP_PLAN[nd].startswith("fused:") for b in FUSED_BATCHES for nd in b)
    assert sorted(set(LONGFFT_BATCH) - {48, 74, 1024}) == LONGFFT_ND
    assert sorted(set(BLUESTEIN_BATCH) - {150, 247}) == BLUESTEIN_ND
    assert all(16 <= len(b) <= 24 for b in FUSED_BATCHES + [LONGFFT_BATCH])
    for b in (FUSED_BATCHES[1], FUSED_BATCHES[4], LONGFFT_BATCH):
        assert any(x == y for x, y in zip(b, b[1:]))
    # the chirp-z groups: packed and unpacked, L = 2^k and 3 * 2^k, one group of two recordings
    assert _blu_groups(BLUESTEIN_ND) == {(False, 48): [17, 23], (False, 128): [63], (True, 6144): [4106],
                                         (False, 24576): [12101]}
    assert {SWEEP_PLAN[nd].split(":")[0] for nd in CROSS_BATCH} == {"fused", "longfft", "bluestein"}


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(len(FUSED_BATCHES)))
def test_fused_lengths(det, record_property, b):
    """Every plan branch of k_hilbert_env: the constant tables (3 ... 29, with
    L == 1 and L > 1), the MFMA stage for each of its primes, Rader 197, the
    register-held direct DFT, 0 ... 13 radix-2 stages, per = 1 ... 20."""
    _sweep(det, record_property, FUSED_BATCHES[b], seed0=FUSED_SEED0[b])


@pytest.mark.gpu
def test_longfft_lengths(det, record_property):
    """The four-step DFT at the short lengths the fused kernel leaves to it:
    packed and unpacked, direct / Rader / in-workgroup Bluestein rows,
    templated and generic radices over one and over several rows per workgroup,
    one-point rows (B == 1: M a prime above 64); with fused lengths in the same
    batch (k_native_yd skips their tiles)."""
    _sweep(det, record_property, LONGFFT_BATCH, seed0=1201)


@pytest.mark.gpu
def test_chirpz_lengths(det, record_property):
    """The lengths neither plan takes, through rocFFT chirp-z (see _blu_groups
    for its choice of L), in one batch with a fused and a long-FFT length."""
    _sweep(det, record_property, BLUESTEIN_BATCH, seed0=1300)


@pytest.mark.gpu
def test_rocfft_cross_check(det, record_property):
    """One batch also through the per-length rocFFT R2C / C2R path
    (OPT_HILBERT_ROCFFT | OPT_HILBERT_R2C), held to the same bound: that run
    shares no transform code with the project's kernels, so it checks the
    host reference itself."""
    from bpm_analysis_amd import _native as N
    nds = CROSS_BATCH
    with_y, refs = _sweep(det, record_property, nds, seed0=1350)
    recs = [_recording(1350 + i, nd * DS - (i % 3)) for i, nd in enumerate(nds)]
    r2c, prof = _profiled(det, recs, FS, dict(G.BASE_PARAMS), want_y=True,
                          options=N.OPT_HILBERT_ROCFFT | N.OPT_HILBERT_R2C)
    assert prof.get("rocfft_r2c", 0) == len(nds)
    assert not any(k in prof for k in ("k_hilbert_env", "k_lf_mid", "k_blu_pre"))
    worst = 0.0
    for nd, a, b, ref in zip(nds, r2c, with_y, refs):
        assert _same(a["y"], b["y"]), nd
        worst = max(worst, float(np.max(np.abs(a["env"] - ref)) / np.max(np.abs(ref))))
    record_property("max_rel_err[rocfft r2c]", worst)
    print(f"rocFFT R2C / C2R: max|env - ref| / max|ref| = {worst:.3e}")
    for nd, a, ref in zip(nds, r2c, refs):
        assert np.max(np.abs(a["env"] - ref)) <= TOL * np.max(np.abs(ref)), nd


@pytest.mark.gpu
@pytest.mark.parametrize("ds,sr,window", [(140, 315, 31), (20, 2205, 220), (146, 302, 30)])
def test_window_geometry(det, record_property, ds, sr, window):
    """Other rolling-mean windows through downsample_factor at 44,100 Hz: an
    odd window (31), one of 220 samples, the default; at Nd from 16 up, so
    windows longer than the recording and windows that straddle the threads'
    runs of `per` outputs.  At sr = 2,205 the band-pass's stop band (above
    150 Hz) lies inside the decimated band, so the bins there are small by
    design (4e-6 of the largest) and the flatness precondition is not made;
    what this test varies is the rolling mean, not the transform."""
    params = dict(G.BASE_PARAMS, downsample_factor=ds)
    d = O.derive(FS, params)
    assert (d.ds, d.sr, d.env_w) == (ds, sr, window)
    assert window > GEOMETRY_ND[0] and -(-GEOMETRY_ND[-1] // 1024) < window
    _sweep(det, record_property, GEOMETRY_ND, params=params, fs_ds=ds, seed0=1400 + ds, fy=ds == DS,
           flat=None if ds == 20 else FLAT)
