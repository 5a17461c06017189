"""Native mode's block-kernel plan (csrc/bpmx_native_plan.h), read without a
GPU: tests/native_plan_driver.hip is compiled as a host program and prints,
for a sample format, channel count, decimation, option bits, PCM alignment and
batch size, which of the eight k_native_blocks kernels the host launches, the
tile length bt and the launch's sizes; and for a recording length which form
k_native_carry's tail and tile scan take.

(a) pins the route and bt on both sides of every switch: mono ds + 1 = 96/97,
160/161, 320/321, 640/641; stereo 2 (ds + 1) = 320/322, 640/642; 16-byte and
4-byte alignment of the PCM; the two option bits; NAT_DSMAX; the generic tile
length min(64, (NB_RCH 512 - 16) / ds).  The expected values are the launch
function's as it stood before the plan was split out of it.

(b) NATIVE_CASES is the table tests/test_gpu_native_formats.py runs on the
GPU, each case with the route and bt it is meant to take.  The driver confirms
every entry, and the table must cover everything the plan can produce for
ds in DS_LO..NAT_DSMAX (`all:`): every route, every instantiation of the
generic kernel (with the int16 stereo kernel's staged and direct branches),
tile lengths of 64, below 64 even, and odd, both tail forms and both forms of
the carry scan.  A plan change that opens a new branch fails here until a
case is added."""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

OPT_NATIVE_F64, OPT_NATIVE_DMA = 2, 128
E_LIMIT = -3
NAT_DSMAX, NAT_TT_PAR, NAT_CPF = 1280, 320, 8
DS_LO = 31                        # fs = 320 ds gives exactly that ds, sr 320 and window 32 from here on
ITEM = {"u8": 1, "i16": 2, "i32": 4, "f32": 4, "f64": 8}
TOTAL = 1 << 20                   # a batch size beyond every threshold

ROUTES = ["mfma<3>", "mfma<5>", "big<5>", "big<10>", "dma<1>", "dma<2>", "i16", "gen"]
GEN_FORMS = [f"gen:{dt}:{m}:direct" for dt in ITEM for m in ("mono", "multi")] + ["gen:i16:multi:staged"]

# name, sample format, channels, ds, option bits, offset of the PCM in
# elements past a 16-byte boundary, the route and bt the case is for, blocks
# of its long recording (1,499: Nd = 1,500 takes the fused Hilbert kernel,
# which makes yd of the full tiles itself in a run without y)
Case = namedtuple("Case", "name dtype ch ds opt off route bt nlong", defaults=(1499,))


def _formats():
    out = []
    for dt in ("u8", "i32", "f32", "f64"):
        for ch in (1, 2, 3):
            out.append(Case(f"{dt}x{ch}", dt, ch, 146, 0, 0, f"gen:{dt}:{'mono' if ch == 1 else 'multi'}:direct", 64))
    return out


NATIVE_CASES = _formats() + [
    # int16 off the matrix-core and DMA kernels
    Case("i16x3", "i16", 3, 146, 0, 0, "gen:i16:multi:direct", 64),
    Case("i16x2+1", "i16", 2, 146, 0, 1, "gen:i16:multi:direct", 64),     # not 4-byte aligned
    Case("i16x2+2", "i16", 2, 146, 0, 2, "gen:i16:multi:staged", 64),     # 4-byte aligned, not 16
    Case("i16x1+1", "i16", 1, 146, 0, 1, "gen:i16:mono:direct", 64),
    # other decimations through the generic kernel: the smallest, an odd and a small tile
    Case("u8x1/31", "u8", 1, 31, 0, 0, "gen:u8:mono:direct", 64),
    Case("f32x2/640", "f32", 2, 640, 0, 0, "gen:f32:multi:direct", 15),
    Case("f64x1/1280", "f64", 1, 1280, 0, 0, "gen:f64:mono:direct", 7),
    Case("i32x2/320", "i32", 2, 320, 0, 0, "gen:i32:multi:direct", 31),
    # int16 mono on both sides of each switch
    Case("i16x1/95", "i16", 1, 95, 0, 0, "mfma<3>", 64),
    Case("i16x1/96", "i16", 1, 96, 0, 0, "mfma<5>", 64),
    Case("i16x1/159", "i16", 1, 159, 0, 0, "mfma<5>", 57),
    Case("i16x1/160", "i16", 1, 160, 0, 0, "big<5>", 64),
    Case("i16x1/319", "i16", 1, 319, 0, 0, "big<5>", 64),
    Case("i16x1/320", "i16", 1, 320, 0, 0, "big<10>", 64),
    Case("i16x1/639", "i16", 1, 639, 0, 0, "big<10>", 60),
    Case("i16x1/640", "i16", 1, 640, 0, 0, "i16", 15),
    # int16 stereo likewise; from 2 (ds + 1) = 642 on the LDS-DMA kernel, up to NAT_DSMAX
    Case("i16x2/159", "i16", 2, 159, 0, 0, "big<5>", 64),
    Case("i16x2/160", "i16", 2, 160, 0, 0, "big<10>", 64),
    Case("i16x2/319", "i16", 2, 319, 0, 0, "big<10>", 60),
    Case("i16x2/320", "i16", 2, 320, 0, 0, "dma<2>", 27),
    Case("i16x2/1280", "i16", 2, 1280, 0, 0, "dma<2>", 3),
    Case("i16x1/dma", "i16", 1, 146, OPT_NATIVE_DMA, 0, "dma<1>", 32),
    # more than 64 NAT_CPF full tiles in the long recording: the carry scan's chunked form
    Case("u8x1/1278", "u8", 1, 1278, 0, 0, "gen:u8:mono:direct", 8, 4201),
    # partners of SAME_TABLE_PAIRS
    Case("i16x2/159+1", "i16", 2, 159, 0, 1, "gen:i16:multi:direct", 64),
    Case("u8x1/95", "u8", 1, 95, 0, 0, "gen:u8:mono:direct", 64),
]
CASES = {c.name: c for c in NATIVE_CASES}

# Two cases with the same ds and bt, hence the same block and tile tables,
# that differ in route or format: run back to back in both orders, a stale or
# wrongly shared cached table shows (the big-K kernel's fragments are keyed
# by key16 alone)
SAME_TABLE_PAIRS = [("i16x2/159", "i16x2/159+1"), ("i16x1/95", "u8x1/95")]


def case_lengths(c):
    """Frames of a case's recordings: 15 blocks (nd = 16: a partial tile only)
    with one tail sample; m bt blocks exactly with a tail of ds samples;
    m bt + 1 blocks with a tail of 1; (m + 1) bt - 1 blocks with a tail of 2;
    the long recording with a tail near ds / 2; and an inactive one of 15 ds
    frames (nd = 15).  m = 2, or what it takes for m bt >= 16 blocks where
    the tile is shorter than 8."""
    m = max(2, -(-16 // c.bt))
    return [15 * c.ds + 1, m * c.bt * c.ds + c.ds, (m * c.bt + 1) * c.ds + 1, ((m + 1) * c.bt - 1) * c.ds + 2,
            c.nlong * c.ds + max(1, c.ds // 2), 15 * c.ds]


def plan_arg(c, total=TOTAL):
    return f"{c.dtype}:{c.ch}:{c.ds}:{c.opt}:{(c.off * ITEM[c.dtype]) % 16}:{total}"


def label(p):
    """A plan line's route as NATIVE_CASES names it."""
    return p["route"] + (":" + p["gen"] if p["route"] == "gen" else "")


def bt_class(bt):
    return "bt=64" if bt == 64 else "bt:odd" if bt % 2 else "bt:even"


def build_driver(workdir):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(workdir), "native_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-o", exe,
                        os.path.join(HERE, "native_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *[str(c) for c in cases]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def parse(line):
    d = dict(kv.split("=", 1) for kv in line.split())
    return {k: (v if k in ("route", "gen", "tail", "scan") else int(v)) for k, v in d.items()}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("native_plan"))


def _plan(driver, dtype, ch, ds, opt=0, align=0, total=TOTAL):
    (ln,) = driver(f"{dtype}:{ch}:{ds}:{opt}:{align}:{total}")
    p = parse(ln)
    assert p["rc"] == 0
    assert p["gstr"] == -(-p["bt"] // 16) * 16 and p["key15"] == p["bt"]
    return p


def _is(p, route, bt, **more):
    assert (label(p), p["bt"]) == (route, bt), p
    for k, v in more.items():
        assert p[k] == v, (k, p)


def test_constants_match_the_library(driver):
    from bpm_analysis_amd import _native as N
    assert (N.OPT_NATIVE_F64, N.OPT_NATIVE_DMA, N.E_LIMIT) == (OPT_NATIVE_F64, OPT_NATIVE_DMA, E_LIMIT)
    assert parse(driver("limits")[0]) == {"dsmax": NAT_DSMAX, "tt_par": NAT_TT_PAR, "cpf": NAT_CPF}
    assert [N.DT_U8, N.DT_I16, N.DT_I32, N.DT_F32, N.DT_F64] == list(range(5))


def test_int16_mono_switches(driver):
    """ds + 1 = 96 / 97: three or five K steps of 32 on the matrix cores;
    160 / 161: the big-K kernel with five K steps of 64; 320 / 321: ten;
    640 / 641: the f64 VALU kernel.  No mono plan has dynamic LDS or a key16
    off the big-K kernel."""
    big = 2 * 19 * 4 * 1024                                    # NB_SLOTS NB_NDMA NB_WAVES KiB
    _is(_plan(driver, "i16", 1, 31), "mfma<3>", 64, lds=0, key16=0)
    _is(_plan(driver, "i16", 1, 95), "mfma<3>", 64, mfma_ks=3)
    _is(_plan(driver, "i16", 1, 96), "mfma<5>", 64, mfma_ks=5, key16=0, lds=0)
    # the 18-KiB slot: ((9216 - 7 - 160 - 2) / ds + 1 blocks
    _is(_plan(driver, "i16", 1, 143), "mfma<5>", 64)
    _is(_plan(driver, "i16", 1, 144), "mfma<5>", 63)
    _is(_plan(driver, "i16", 1, 146), "mfma<5>", 62)
    _is(_plan(driver, "i16", 1, 159), "mfma<5>", 57)
    _is(_plan(driver, "i16", 1, 160), "big<5>", 64, big_ks=5, big_bs=16, key16=1005, lds=big, mfma_ks=0)
    _is(_plan(driver, "i16", 1, 319), "big<5>", 64, key16=1005)
    _is(_plan(driver, "i16", 1, 320), "big<10>", 64, big_ks=10, big_bs=16, key16=1010, lds=big)
    # the 19-KiB slot: 16 blocks per sub-tile while (9728 - 7 - 640 - 2) / ds >= 15
    _is(_plan(driver, "i16", 1, 605), "big<10>", 64, big_bs=16)
    _is(_plan(driver, "i16", 1, 606), "big<10>", 60, big_bs=15)
    _is(_plan(driver, "i16", 1, 639), "big<10>", 60, big_bs=15, key16=1010)
    _is(_plan(driver, "i16", 1, 640), "i16", 15, big_ks=0, key16=0, lds=0)
    _is(_plan(driver, "i16", 1, NAT_DSMAX), "i16", 7)


def test_int16_stereo_switches(driver):
    """2 (ds + 1) = 320 / 322: five or ten K steps; 640 / 642: the LDS-DMA
    kernel, whose tile is what its LDS slot holds.  nd_tile_blocks stays >= 1
    up to NAT_DSMAX, so no aligned int16 stereo batch falls to the generic
    kernel."""
    _is(_plan(driver, "i16", 2, 31), "big<5>", 64, key16=2005)
    _is(_plan(driver, "i16", 2, 159), "big<5>", 64, big_bs=16, key16=2005)
    _is(_plan(driver, "i16", 2, 160), "big<10>", 64, big_bs=16, key16=2010)
    _is(_plan(driver, "i16", 2, 302), "big<10>", 64, big_bs=16)
    _is(_plan(driver, "i16", 2, 303), "big<10>", 60, big_bs=15)
    _is(_plan(driver, "i16", 2, 319), "big<10>", 60, big_bs=15, key16=2010)
    # 34 KiB per slot at ds = 320: ((34 * 512 - 7) / 2 - 1) / 320 = 27 blocks
    _is(_plan(driver, "i16", 2, 320), "dma<2>", 27, ndma=34, key16=0, lds=34 * 4096 + 321 * 64 + 45 * 8)
    _is(_plan(driver, "i16", 2, 600), "dma<2>", 12, ndma=30)
    _is(_plan(driver, "i16", 2, NAT_DSMAX), "dma<2>", 3, ndma=19, lds=19 * 4096 + 1281 * 64 + 45 * 8)
    plans = [parse(ln) for ln in driver(*[f"i16:2:{ds}:0:0:{TOTAL}" for ds in range(1, NAT_DSMAX + 1)])]
    assert all(p["route"] in ("big<5>", "big<10>", "dma<2>") and p["bt"] >= 1 for p in plans)
    assert all(p["lds"] <= 160 * 1024 for p in plans)
    # three channels: nothing but the generic kernel
    _is(_plan(driver, "i16", 3, 100), "gen:i16:multi:direct", 64)


def test_options(driver):
    """BPMX_OPT_NATIVE_F64: the f64 VALU kernels (k_native_blocks_i16 for mono,
    the generic kernel's staged branch for stereo); BPMX_OPT_NATIVE_DMA: the
    LDS-DMA kernel for mono too, two lanes per block, so at most 32 blocks;
    F64 wins over DMA."""
    for ds in (95, 146, 300, 640):
        bt = min(64, (20 * 512 - 16) // ds)
        _is(_plan(driver, "i16", 1, ds, OPT_NATIVE_F64), "i16", bt, lds=0, key16=0)
        _is(_plan(driver, "i16", 2, ds, OPT_NATIVE_F64), "gen:i16:multi:staged", bt, lds=0, key16=0)
        _is(_plan(driver, "i16", 1, ds, OPT_NATIVE_F64 | OPT_NATIVE_DMA), "i16", bt)
        _is(_plan(driver, "i16", 2, ds, OPT_NATIVE_F64 | OPT_NATIVE_DMA), "gen:i16:multi:staged", bt)
    _is(_plan(driver, "i16", 1, 95, OPT_NATIVE_DMA), "dma<1>", 32, ndma=38)
    _is(_plan(driver, "i16", 1, 146, OPT_NATIVE_DMA), "dma<1>", 32, ndma=37, lds=37 * 4096 + 147 * 64 + 45 * 8)
    _is(_plan(driver, "i16", 1, 640, OPT_NATIVE_DMA), "dma<1>", 23, ndma=29)
    _is(_plan(driver, "i16", 2, 146, OPT_NATIVE_DMA), "dma<2>", 32)       # stereo: no matrix cores on request
    _is(_plan(driver, "i16", 2, 400, OPT_NATIVE_DMA), "dma<2>", 21)
    for dt in ("u8", "i32", "f32", "f64"):                                # other formats: the bits change nothing
        for opt in (OPT_NATIVE_F64, OPT_NATIVE_DMA):
            assert _plan(driver, dt, 1, 146, opt) == _plan(driver, dt, 1, 146)


def test_alignment_and_batch_size(driver):
    """The matrix-core, DMA and int16 VALU kernels load 16-byte chunks: a PCM
    address off a 16-byte boundary sends int16 to the generic kernel, whose
    stereo branch stages dwords in LDS when the address is 4-byte aligned.  A
    batch of fewer than 16 elements has no whole chunk."""
    for align in range(2, 16, 2):
        _is(_plan(driver, "i16", 1, 146, 0, align), "gen:i16:mono:direct", 64)
        _is(_plan(driver, "i16", 1, 146, OPT_NATIVE_DMA, align), "gen:i16:mono:direct", 64)
        _is(_plan(driver, "i16", 2, 146, 0, align), "gen:i16:multi:" + ("direct" if align % 4 else "staged"), 64)
        _is(_plan(driver, "i16", 2, 400, 0, align), "gen:i16:multi:" + ("direct" if align % 4 else "staged"), 25)
        _is(_plan(driver, "i16", 3, 146, 0, align), "gen:i16:multi:direct", 64)
    _is(_plan(driver, "i16", 1, 146, 0, 0, 16), "mfma<5>", 62)
    _is(_plan(driver, "i16", 1, 146, 0, 0, 15), "i16", 64)
    _is(_plan(driver, "i16", 2, 146, 0, 0, 16), "big<5>", 64)
    _is(_plan(driver, "i16", 2, 146, 0, 0, 14), "gen:i16:multi:staged", 64)
    _is(_plan(driver, "i16", 1, 146, OPT_NATIVE_DMA, 0, 15), "i16", 64)
    for dt in ("u8", "i32", "f32", "f64"):                                # element loads: any alignment
        for align in range(0, 16, ITEM[dt]):
            _is(_plan(driver, dt, 2, 146, 0, align), f"gen:{dt}:multi:direct", 64)


def test_generic_tile_length_and_limit(driver):
    """bt = min(64, (NB_RCH 512 - 16) / ds) on the generic and int16 VALU
    kernels: 64 up to ds = 159, 63 (below 64 and odd at once) at 160, the
    first even one below 64 at 164; NAT_DSMAX is the last ds, beyond it
    BPMX_E_LIMIT."""
    for dt, ch in (("u8", 1), ("i32", 2), ("f32", 3), ("f64", 1)):
        form = f"gen:{dt}:{'mono' if ch == 1 else 'multi'}:direct"
        for ds, bt in ((1, 64), (31, 64), (159, 64), (160, 63), (163, 62), (164, 62), (165, 61), (640, 15),
                       (1278, 8), (1279, 7), (NAT_DSMAX, 7)):
            assert bt == min(64, 10224 // ds)
            _is(_plan(driver, dt, ch, ds), form, bt, lds=0, key16=0)
        assert parse(driver(f"{dt}:{ch}:{NAT_DSMAX + 1}:0:0:{TOTAL}")[0]) == {"rc": E_LIMIT}
    assert parse(driver(f"i16:1:{NAT_DSMAX + 1}:0:0:{TOTAL}")[0]) == {"rc": E_LIMIT}
    assert parse(driver(f"i16:2:{NAT_DSMAX + 1}:{OPT_NATIVE_DMA}:0:{TOTAL}")[0]) == {"rc": E_LIMIT}


def test_tail_and_scan_forms(driver):
    """k_native_carry's tail holds the samples from the last decimated one on
    (1 ... ds) and the 15 of the right pad; up to NAT_TT_PAR of them go lane-
    parallel.  Its tile scan keeps up to NAT_CPF tiles per lane in registers:
    512 full tiles, chunks beyond."""
    def rec(ds, bt, n):
        return parse(driver(f"rec:{ds}:{bt}:{n}")[0])
    assert rec(146, 64, 146 * 15 + 1) == dict(nd=16, nb=15, tf=0, lp=15, nt=16, tail="par", scan="reg")
    assert rec(146, 64, 146 * 129) == dict(nd=129, nb=128, tf=2, lp=0, nt=161, tail="par", scan="reg")
    assert rec(1280, 7, 1280 * 20 + 305)["tail"] == "par" and rec(1280, 7, 1280 * 20 + 305)["nt"] == NAT_TT_PAR
    assert rec(1280, 7, 1280 * 20 + 306)["tail"] == "serial"
    assert rec(1280, 7, 1280 * 21)["nt"] == 1295
    assert rec(146, 8, 146 * 8 * 512 + 1) == dict(nd=4097, nb=4096, tf=512, lp=0, nt=16, tail="par", scan="reg")
    assert rec(146, 8, 146 * (8 * 513 - 1) + 1)["scan"] == "reg"
    assert rec(146, 8, 146 * 8 * 513 + 1) == dict(nd=4105, nb=4104, tf=513, lp=0, nt=16, tail="par", scan="chunked")


def _case_branches(driver, c):
    """What a case runs: (route label, bt class, tail forms, scan forms)."""
    recs = [parse(ln) for ln in driver(*[f"rec:{c.ds}:{c.bt}:{n}" for n in case_lengths(c)])]
    active = [r for r in recs if r["nd"] > 15]
    return recs, {r["tail"] for r in active}, {r["scan"] for r in active}


def test_cases_are_what_the_plan_says(driver):
    """Every NATIVE_CASES entry takes the route and bt it names, and its
    recordings have the shapes the GPU test relies on."""
    assert len(CASES) == len(NATIVE_CASES)
    plans = [parse(ln) for ln in driver(*[plan_arg(c) for c in NATIVE_CASES])]
    for c, p in zip(NATIVE_CASES, plans):
        assert p["rc"] == 0 and (label(p), p["bt"]) == (c.route, c.bt), (c, p)
        assert DS_LO <= c.ds <= NAT_DSMAX
        lens = case_lengths(c)
        # the smallest batch a test may run (one active recording) is planned alike
        assert parse(driver(plan_arg(c, total=lens[0] * c.ch))[0]) == p
        recs, _, _ = _case_branches(driver, c)
        m = max(2, -(-16 // c.bt))
        assert [(r["nd"], r["tf"], r["lp"], r["nt"] - 15) for r in recs[:4]] == [
            (16, 0, 15, 1) if c.bt > 15 else (16, 15 // c.bt, 15 % c.bt, 1),
            (m * c.bt + 1, m, 0, c.ds), (m * c.bt + 2, m, 1, 1), ((m + 1) * c.bt, m, c.bt - 1, 2)], c
        assert recs[4]["nb"] == c.nlong and recs[4]["nt"] - 15 == max(1, c.ds // 2)
        assert recs[5]["nd"] == 15                              # inactive: filtfilt's padlen
    for a, b in SAME_TABLE_PAIRS:
        pa, pb = (parse(driver(plan_arg(CASES[n]))[0]) for n in (a, b))
        assert CASES[a].ds == CASES[b].ds and pa["bt"] == pb["bt"] and label(pa) != label(pb)


def test_cases_cover_every_plan_branch(driver):
    everything = {ln.rsplit(" ", 1)[0] for ln in driver(f"all:{DS_LO}-{NAT_DSMAX + 1}")}
    assert everything == set(ROUTES[:-1]) | set(GEN_FORMS) | {"bt=64", "bt:even", "bt:odd", "limit"}
    covered = {c.route for c in NATIVE_CASES} | {bt_class(c.bt) for c in NATIVE_CASES}
    assert covered == everything - {"limit"}, sorted(everything - covered)
    tails, scans = set(), set()
    for c in NATIVE_CASES:
        _, t, s = _case_branches(driver, c)
        tails |= t
        scans |= s
    assert tails == {"par", "serial"} and scans == {"reg", "chunked"}
    # the two int16 VALU forms BPMX_OPT_NATIVE_F64 adds to the int16 cases
    f64 = {label(parse(driver(plan_arg(c._replace(opt=OPT_NATIVE_F64)))[0])) for c in NATIVE_CASES
           if c.dtype == "i16" and c.off == 0}
    assert f64 == {"i16", "gen:i16:multi:staged", "gen:i16:multi:direct"}


if __name__ == "__main__":                                    # print the table's plans
    import tempfile
    run = build_driver(tempfile.mkdtemp())
    for c in NATIVE_CASES:
        print(c.name, run(plan_arg(c))[0])
