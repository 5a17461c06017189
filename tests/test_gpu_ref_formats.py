"""Reference mode's envelope (k_ref_pick -> k_ref_fwd -> k_envelope_ref_t ->
k_ref_kahan -> k_ref_env_mean) against the oracle, bit for bit, over the cases
of tests/ref_cases.py: every envelope window that selects another
kahan_chain<W>, every sample format with one to three channels, ragged
batches of 70 recordings (two waves, a row stride that is no multiple of 64)
whose lengths sit on the forward pass's and the Kahan pass's row-chunk ends,
runs of equal |y|, subnormal samples, and NaN / Inf recordings beside clean
ones.  tests/test_ref_cases.py keeps the table a cover, proves the length sets
sit on the plan's switches and pins the oracle on these inputs against scipy
and pandas, all without a GPU.

A case runs as one device buffer with 64 guard elements of the format's
largest finite value before and after the batch, which starts 0 or an odd
number of elements behind the front guard; the guards are read back unchanged.
Detector.run keeps the given order (run_host would sort the recordings by
length and move them between waves).  Nothing here has a tolerance."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ref_cases as RC
from tests.test_gpu_hilbert_lengths import _oracle_answer
from tests.test_gpu_native_formats import _assert_inactive, _assert_same_runs
from tests.test_gpu_params import _check
from tests.test_plan import OPT_REF_NOSPLIT, OPT_REF_SERIAL_MEAN

GUARD = 64
D_INT, D_F32 = 1e-3, 3e-9
ALL_KEYS = ("y", "env", "floor", "troughs", "peaks")


@pytest.fixture(scope="module")
def det():
    from bpm_analysis_amd.engine import Detector
    return Detector(0)


class Buffer:
    """A batch on the device between its guards."""

    def __init__(self, det, recs, ch, off):
        import torch
        self.det, self.ch, self.off = det, ch, off
        dt = recs[0].dtype
        assert all(r.dtype == dt and (r.ndim == 1 if ch == 1 else r.shape[1] == ch) for r in recs)
        self.top = np.iinfo(dt).max if dt.kind in "iu" else np.finfo(dt).max
        flat = np.concatenate([np.full(GUARD + off, self.top, dt)] + [r.reshape(-1) for r in recs] +
                              [np.full(GUARD, self.top, dt)])
        self.fo = np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])]).astype(np.int64)
        self.dev = torch.from_numpy(flat).to(det.device)
        assert self.dev.data_ptr() % 16 == 0
        self.end = GUARD + off + int(self.fo[-1]) * ch
        assert self.end + GUARD == flat.size

    def run(self, fs, params, want_y=True, options=0):
        import torch
        pcm = self.dev[GUARD + self.off:self.end]
        res = self.det.run(pcm, self.fo, fs, params, mode="reference", channels=self.ch, want_y=want_y,
                           options=options)
        torch.cuda.synchronize()
        out = res.to_host()
        front, back = self.dev[:GUARD + self.off].cpu().numpy(), self.dev[self.end:].cpu().numpy()
        assert back.size == GUARD and np.all(front == self.top) and np.all(back == self.top)
        return out


def _answers(recs, w):
    """The oracle's y, env and detection per recording (None where nd <= 15;
    no detection on an envelope with a NaN)."""
    fs, ds, _ = RC.RATES[w]
    d, p = RC.derived(w), RC.params(w)
    out = []
    for x in recs:
        if RC.nd_of(x, ds) <= 15:
            out.append(None)
            continue
        env, y = O.preprocess_ref(x, d, return_y=True)
        out.append(dict(env=env, y=y) if np.isnan(env).any() else dict(_oracle_answer(env, p, fs), y=y))
    return out


def _assert_inputs_discriminate(c, recs, ans):
    """The conditions of tests/test_ref_cases.py's docstring, on this case's own recordings."""
    d = RC.derived(c.rate)
    integer = c.dtype in ("u8", "i16", "i32")
    for k, (x, o) in enumerate(zip(recs, ans)):
        if o is None:
            continue
        dist = RC.discrimination(o["y"], RC.cast_y(x, d))
        if integer and c.ch == 1:
            assert dist >= D_INT, (c.name, k, dist)
        elif integer:
            x0 = np.ascontiguousarray(x[:, 0])
            d0 = RC.discrimination(O.preprocess_ref(x0, d, return_y=True)[1], RC.cast_y(x0, d))
            assert dist == 0.0 and d0 >= D_INT, (c.name, k, dist, d0)
        elif c.dtype == "f32":
            assert dist >= D_F32, (c.name, k, dist)
        else:
            assert dist == 0.0, (c.name, k)


_cache = {}                         # case name -> the oracle's answers
_last = {}                          # the recordings of the case run last (a kahan set is up to 170 MB)


def _case_inputs(c):
    if _last.get("name") != c.name:
        _last.clear()
        _last.update(name=c.name, recs=RC.case_recordings(c))
    recs = _last["recs"]
    if c.name not in _cache:
        ans = _answers(recs, c.rate)
        _assert_inputs_discriminate(c, recs, ans)
        _cache[c.name] = ans
    return recs, _cache[c.name]


def _check_envelope(r, o, sr, what):
    """sr, lengths, y and env bit for bit."""
    assert r["sr"] == sr, what
    assert r["y"].size == r["env"].size == o["y"].size == o["env"].size, what
    assert np.array_equal(r["y"], o["y"], equal_nan=True), ("y", what)
    assert np.array_equal(r["env"], o["env"], equal_nan=True), ("env", what)


def _check_against_oracle(res, ans, sr, name):
    assert len(res) == len(ans)
    for k, (r, o) in enumerate(zip(res, ans)):
        if o is None:
            _assert_inactive(r, (name, k))
            continue
        _check_envelope(r, o, sr, (name, k, o["y"].size))
        _check(r, o, (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in RC.REF_CASES])
def test_ref_case(det, name):
    c = RC.CASES[name]
    fs, _, sr = RC.RATES[c.rate]
    p = RC.params(c.rate)
    recs, ans = _case_inputs(c)
    assert sum(o is None for o in ans) == 1
    buf = Buffer(det, recs, c.ch, c.off)
    first = buf.run(fs, p)
    _check_against_oracle(first, ans, sr, name)
    plain = buf.run(fs, p, want_y=False)
    assert all(r["y"] is None for r in plain)
    _assert_same_runs(plain, first, (name, "no y"))
    for opt in (OPT_REF_NOSPLIT, OPT_REF_SERIAL_MEAN):
        _assert_same_runs(buf.run(fs, p, options=opt), first, (name, opt), keys=ALL_KEYS)


def _with_specials(base, specials):
    """`base` with `specials` {index: recording} put in (indices of the result)."""
    out = list(base)
    for i in sorted(specials):
        out.insert(i, specials[i])
    return out


def _split_recordings(w, dtype, ch, seed0):
    fs, ds, _ = RC.RATES[w]
    return [RC.recording(dtype, ch, nd, ds, seed0 + i, "max" if i % 2 else "min", fs)
            for i, nd in enumerate(RC.set_nds("split", w))]


def _run_default_and_serial(det, recs, ch, w, name):
    fs, _, sr = RC.RATES[w]
    p = RC.params(w)
    ans = _answers(recs, w)
    buf = Buffer(det, recs, ch, 1)
    for opt in (0, OPT_REF_SERIAL_MEAN):
        res = buf.run(fs, p, options=opt)
        assert len(res) == len(ans)
        for k, (r, o) in enumerate(zip(res, ans)):
            if o is None:
                _assert_inactive(r, (name, k))
            else:
                _check_envelope(r, o, sr, (name, opt, k))
    return ans


@pytest.mark.gpu
@pytest.mark.parametrize("w", list(RC.RATES))
def test_equal_runs_and_subnormals(det, w):
    """Runs of equal |y| shorter and longer than the window (few_ulp), float64
    and float32 subnormals and an all-zero recording among ordinary ones, in
    both waves: chain mode's count of the run that ends at the last added
    value (k_ref_env_mean) and the in-pass RollMean (BPMX_OPT_REF_SERIAL_MEAN)
    both equal the oracle, and nothing is flushed to zero."""
    fs, ds, _ = RC.RATES[w]
    few, sub = RC.few_ulp_for(w), RC.subnormal_f64(3, fs)
    recs = _with_specials(_split_recordings(w, "f64", 1, 52000),
                          {1: few, 10: sub, 20: np.zeros(12 * fs), 70: sub.copy(), 72: few.copy()})
    assert len(recs) == 75 and recs[72] is not few
    ans = _run_default_and_serial(det, recs, 1, w, f"w{w} f64")
    assert RC.few_ulp_condition(ans[1]["y"], w) and np.all(ans[20]["env"] == 0)
    assert 0 < np.max(np.abs(ans[10]["y"])) < RC.DBL_MIN
    for ch in (1, 2):
        s32 = RC.subnormal_f32(4, fs, ch)
        recs = _with_specials(_split_recordings(w, "f32", ch, 53000 + ch), {5: s32, 68: s32.copy()})
        ans = _run_default_and_serial(det, recs, ch, w, f"w{w} f32x{ch}")
        assert 0 < np.max(np.abs(ans[5]["y"])) < RC.FLT_MIN


NONFINITE_BATCHES = [(w, dt) for w in (31, 44, 220) for dt in ("f32", "f64")]


@pytest.mark.gpu
@pytest.mark.parametrize("w,dtype", NONFINITE_BATCHES, ids=[f"w{w}-{dt}" for w, dt in NONFINITE_BATCHES])
def test_nonfinite_neighbours(det, w, dtype):
    """A NaN or +Inf recording at lanes 3 and 40 of wave 0: its y and env are
    NaN throughout, as the oracle's; wave 0 leaves chain mode, so its clean
    recordings take k_envelope_ref_t's in-pass means, wave 1 stays in chain
    mode, and every clean recording equals the oracle bit for bit."""
    fs, ds, sr = RC.RATES[w]
    p = RC.params(w)
    recs = _split_recordings(w, dtype, 1, 54000)
    bad = {}
    for j, (lane, nd) in enumerate(((3, 1025), (40, 994))):
        kind, pos = RC.NONFINITE[(2 * NONFINITE_BATCHES.index((w, dtype)) + j) % len(RC.NONFINITE)]
        bad[lane] = recs[lane] = RC.nonfinite(kind, pos, dtype, nd, ds, 54100 + j, fs)
    assert len(recs) == 70 and all(np.isfinite(r).all() for k, r in enumerate(recs) if k not in bad)
    ans = _answers(recs, w)
    buf = Buffer(det, recs, 1, 3)
    first = buf.run(fs, p)
    for k, (r, o) in enumerate(zip(first, ans)):
        if o is None:
            _assert_inactive(r, (w, dtype, k))
        elif k in bad:
            assert np.isnan(o["y"]).all() and np.isnan(o["env"]).all()
            _check_envelope(r, o, sr, (w, dtype, k))
            assert np.isnan(r["y"]).all() and np.isnan(r["env"]).all(), (w, dtype, k)
        else:
            _check_envelope(r, o, sr, (w, dtype, k))
            _check(r, o, (w, dtype, k))
    for opt in (OPT_REF_NOSPLIT, OPT_REF_SERIAL_MEAN):
        _assert_same_runs(buf.run(fs, p, options=opt), first, (w, dtype, opt), keys=ALL_KEYS)


def test_nonfinite_batches_use_every_kind_and_place():
    used = {RC.NONFINITE[(2 * b + j) % len(RC.NONFINITE)] for b in range(len(NONFINITE_BATCHES)) for j in (0, 1)}
    assert used == set(RC.NONFINITE) and len(used) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("w", list(RC.RATES))
def test_chunk_edges_do_not_depend_on_neighbours(det, w):
    """Recordings that end on, beside and a half window past the Kahan chunk
    ends of their batch, run alone (their own length then decides the
    chunks): the outputs they had inside the batch, bit for bit."""
    c = RC.CASES[f"w{w}-i16x1-kahan"]
    fs = RC.RATES[w][0]
    p = RC.params(w)
    recs, _ = _case_inputs(c)
    batch = Buffer(det, recs, c.ch, c.off).run(fs, p)
    nds = RC.set_nds(c.set, w)
    ke, off = RC.kend(RC.MAXND), (w - 1) // 2
    for nd in (ke[0], ke[0] + off + 1, ke[1] - 1, ke[2] + 1, RC.MAXND):
        k = nds.index(nd)
        alone = Buffer(det, [recs[k]], c.ch, c.off).run(fs, p)
        assert alone[0]["env"].size == nd
        _assert_same_runs(alone, [batch[k]], (w, nd), keys=ALL_KEYS)
