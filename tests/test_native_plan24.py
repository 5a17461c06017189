"""Native mode's block-kernel plan for packed 24-bit PCM (BPMX_DT_I24), read
without a GPU: tests/native_plan24_driver.hip is compiled as a host program
and prints csrc/bpmx_native_plan.h's plan.

Mono I24 with ds + 1 <= 96 / <= 160 takes k_native_blocks_mfma24<3> / <5> at
any byte alignment once the batch has 16 samples; BPMX_OPT_NATIVE_F64, mono
beyond K = 160, two and more channels and smaller batches take the generic
kernel's I24 instantiation.  Every switch is pinned on both sides, the tile
length at every ds the GPU test runs (P24_CASES, which
tests/test_gpu_pcm24.py imports), and the plans of the five earlier formats
are the ones tests/test_native_plan.py's NATIVE_CASES name."""
import os
import shutil
import subprocess

import pytest

from tests.test_native_plan import (CASES, NAT_DSMAX, OPT_NATIVE_DMA, OPT_NATIVE_F64, TOTAL, Case, case_lengths, label,
                                    parse, plan_arg)

HERE = os.path.dirname(os.path.abspath(__file__))
E_LIMIT = -3
SLOT = 18 * 1024                                              # NM_SLOT_CH 16-byte chunks


def slot_blocks(ds, ks):
    """nm24_tile_blocks: the slot holds up to 15 bytes before the tile, and
    the last block's last K step reads 13 dwords from the dword at or below
    its start: 96 ks + 4 bytes from the block's first.  Even, so that the fused
    Hilbert kernel can make yd of the full tiles."""
    b = (SLOT - 15 - 96 * ks - 4) // (3 * ds) + 1
    return 64 if b >= 64 else b & ~1


# the cases tests/test_gpu_pcm24.py runs: name, format, channels, ds, options, (unused), route, bt
P24_CASES = [
    Case("i24x1/95", "i24", 1, 95, 0, 0, "mfma24<3>", 64),
    Case("i24x1/96", "i24", 1, 96, 0, 0, "mfma24<5>", 62),
    Case("i24x1/146", "i24", 1, 146, 0, 0, "mfma24<5>", 40),
    Case("i24x1/159", "i24", 1, 159, 0, 0, "mfma24<5>", 38),
    Case("i24x1/160", "i24", 1, 160, 0, 0, "gen:i24:mono:direct", 63),
    Case("i24x2/146", "i24", 2, 146, 0, 0, "gen:i24:multi:direct", 64),
]
P24 = {c.name: c for c in P24_CASES}
OFFSETS = (0, 1, 2, 3, 15)                                    # guard bytes beyond GUARD before a batch


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(tmp_path_factory.mktemp("native_plan24")), "native_plan24_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-o", exe,
                        os.path.join(HERE, "native_plan24_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *[str(c) for c in cases]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def _plan(driver, ch, ds, opt=0, align=0, total=TOTAL):
    (ln,) = driver(f"i24:{ch}:{ds}:{opt}:{align}:{total}")
    p = parse(ln)
    assert p["rc"] == 0
    assert p["gstr"] == -(-p["bt"] // 16) * 16 and p["key15"] == p["bt"] and p["lds"] == 0 and p["ndma"] == 0
    return p


def _is(p, route, bt, **more):
    assert (label(p), p["bt"]) == (route, bt), p
    for k, v in more.items():
        assert p[k] == v, (k, p)


def test_constants_match_the_library():
    from bpm_analysis_amd import _native as N
    assert N.DT_I24 == 5 and N.OPT_NATIVE_F64 == OPT_NATIVE_F64
    with open(os.path.join(HERE, "..", "include", "bpmx.h")) as fh:
        assert "BPMX_DT_I24 = 5" in fh.read()


def test_mono_switches(driver):
    """ds + 1 = 96 / 97: three or five K steps; 160 / 161: the generic kernel.
    The 24-bit tables are keyed apart from the int16 ones (key16)."""
    _is(_plan(driver, 1, 1), "mfma24<3>", 64, mfma_ks=3, key16=24)
    _is(_plan(driver, 1, 31), "mfma24<3>", 64)
    _is(_plan(driver, 1, 95), "mfma24<3>", 64, mfma_ks=3, key16=24)
    _is(_plan(driver, 1, 96), "mfma24<5>", 62, mfma_ks=5, key16=24)
    _is(_plan(driver, 1, 159), "mfma24<5>", 38, mfma_ks=5, key16=24)
    _is(_plan(driver, 1, 160), "gen:i24:mono:direct", 63, mfma_ks=0, key16=0)
    _is(_plan(driver, 1, 640), "gen:i24:mono:direct", 15, key16=0)
    _is(_plan(driver, 1, NAT_DSMAX), "gen:i24:mono:direct", 7)
    assert parse(driver(f"i24:1:{NAT_DSMAX + 1}:0:0:{TOTAL}")[0]) == {"rc": E_LIMIT}


def test_tile_length_is_what_the_slot_holds(driver):
    """bt at every ds of the matrix-core routes: 64 while the slot holds them
    (ds <= 94 with three K steps), then fewer; never below 38."""
    plans = [parse(ln) for ln in driver(*[f"i24:1:{ds}:0:5:{TOTAL}" for ds in range(1, 160)])]
    for ds, p in zip(range(1, 160), plans):
        ks = 3 if ds + 1 <= 96 else 5
        assert (p["route"], p["bt"], p["mfma_ks"]) == (f"mfma24<{ks}>", slot_blocks(ds, ks), ks), (ds, p)
        # the tile and the last block's last K step stay inside the slot
        assert 15 + 3 * (p["bt"] * ds + 1) <= SLOT and 15 + 3 * (p["bt"] - 1) * ds + 96 * ks + 4 <= SLOT
        assert 32 * ks >= ds + 1
    assert plans[94 - 1]["bt"] == 64 and plans[95 - 1]["bt"] == 64 and plans[96 - 1]["bt"] == 62
    assert min(p["bt"] for p in plans) == 38 and all(p["bt"] % 2 == 0 for p in plans)
    for c in P24_CASES:
        if c.route.startswith("mfma24"):
            assert c.bt == slot_blocks(c.ds, 3 if c.ds + 1 <= 96 else 5)


def test_channels_and_option(driver):
    """Two and more channels and BPMX_OPT_NATIVE_F64 take the generic kernel;
    BPMX_OPT_NATIVE_DMA means nothing to the format."""
    for ds in (95, 146, 159):
        bt = min(64, 10224 // ds)
        _is(_plan(driver, 2, ds), "gen:i24:multi:direct", bt, key16=0)
        _is(_plan(driver, 3, ds), "gen:i24:multi:direct", bt, key16=0)
        _is(_plan(driver, 1, ds, OPT_NATIVE_F64), "gen:i24:mono:direct", bt, key16=0)
        _is(_plan(driver, 1, ds, OPT_NATIVE_F64 | OPT_NATIVE_DMA), "gen:i24:mono:direct", bt)
        _is(_plan(driver, 2, ds, OPT_NATIVE_F64), "gen:i24:multi:direct", bt)
        assert _plan(driver, 1, ds, OPT_NATIVE_DMA) == _plan(driver, 1, ds)
    _is(_plan(driver, 2, 640), "gen:i24:multi:direct", 15)


def test_alignment_and_batch_size(driver):
    """Any byte alignment keeps the route and bt; a batch below 16 samples
    goes to the generic kernel."""
    for ds in (95, 146):
        base = _plan(driver, 1, ds)
        for align in range(16):
            assert _plan(driver, 1, ds, 0, align) == base
            _is(_plan(driver, 2, ds, 0, align), "gen:i24:multi:direct", 64)
    _is(_plan(driver, 1, 146, 0, 7, 16), "mfma24<5>", 40)
    _is(_plan(driver, 1, 146, 0, 7, 15), "gen:i24:mono:direct", 64, key16=0)
    _is(_plan(driver, 1, 95, 0, 0, 16), "mfma24<3>", 64)
    _is(_plan(driver, 1, 95, 0, 0, 15), "gen:i24:mono:direct", 64)


def test_gpu_cases_are_what_the_plan_says(driver):
    for c in P24_CASES:
        for align in range(16):
            p = parse(driver(f"i24:{c.ch}:{c.ds}:{c.opt}:{align}:{TOTAL}")[0])
            assert p["rc"] == 0 and (label(p), p["bt"]) == (c.route, c.bt), (c, p)
        lens = case_lengths(c)
        assert parse(driver(f"i24:{c.ch}:{c.ds}:0:0:{lens[0] * c.ch}")[0])["route"] == p["route"]
        recs = [parse(ln) for ln in driver(*[f"rec:{c.ds}:{c.bt}:{n}" for n in lens])]
        assert [(r["nd"], r["tf"], r["lp"]) for r in recs[:4]] == [
            (16, 0, 15), (2 * c.bt + 1, 2, 0), (2 * c.bt + 2, 2, 1), (3 * c.bt, 2, c.bt - 1)], c
        assert recs[4]["nb"] == 1499 and recs[5]["nd"] == 15
        # with BPMX_OPT_NATIVE_F64: the generic kernel, tiled as for int32
        f = parse(driver(f"i24:{c.ch}:{c.ds}:{OPT_NATIVE_F64}:0:{TOTAL}")[0])
        g = parse(driver(f"i32:{c.ch}:{c.ds}:0:0:{TOTAL}")[0])
        assert f["route"] == g["route"] == "gen" and f["bt"] == g["bt"] and f["key16"] == g["key16"] == 0


EARLIER = ["u8x1", "i32x1", "i32x2", "f32x3", "f64x1", "i16x3", "i16x2+2", "i16x1+1", "i16x1/95", "i16x1/96", "i16x1/159",
           "i16x1/160", "i16x1/639", "i16x1/640", "i16x2/319", "i16x2/320", "i16x1/dma", "f64x1/1280"]


def test_earlier_formats_plan_as_before(driver):
    """A handful of NATIVE_CASES through this driver: the route and bt the
    table names."""
    lines = driver(*[plan_arg(CASES[n]) for n in EARLIER])
    for n, ln in zip(EARLIER, lines):
        p = parse(ln)
        assert p["rc"] == 0 and (label(p), p["bt"]) == (CASES[n].route, CASES[n].bt), (n, p)
        assert p["key16"] != 24


def test_earlier_driver_prints_the_same_lines(driver, tmp_path):
    from tests.test_native_plan import build_driver
    old = build_driver(tmp_path)
    args = [plan_arg(CASES[n]) for n in EARLIER] + [f"i16:1:146:0:0:{t}" for t in (15, 16)] + \
           [f"{dt}:{ch}:{ds}:{opt}:0:{TOTAL}" for dt in ("u8", "i16", "i32", "f32", "f64") for ch in (1, 2)
            for ds in (95, 96, 159, 160) for opt in (0, OPT_NATIVE_F64)]
    assert driver(*args) == old(*args)
