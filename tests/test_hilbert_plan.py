"""The plans of the device Hilbert transforms, read without a GPU:
tests/hilbert_plan_driver.hip is compiled as a host program around
csrc/k_hilbert.hip and csrc/k_longfft.hip and prints, per decimated length Nd,
which transform the host picks and how that transform is staged.

Native mode's Nd is whatever the user's file length makes it, and the stage
code each transform runs depends on Nd's factorisation.  FUSED_ND and
LONGFFT_ND are the lengths tests/test_gpu_hilbert_lengths.py sweeps on the
GPU; (a) keeps them a cover of every plan branch, so that a plan change which
opens a new branch fails here until a length is added:

* fused kernel (k_hilbert_env): every (odd prime, stage form, L == 1 or
  L > 1), every count of radix-2 stages, every rolling-mean run length `per`.
  Stage forms: cp (constants from bpmx_dft_consts.h), mf (f64 MFMA GEMM),
  rd (Rader 197), gen (register-held direct DFT).
* four-step DFT (k_longfft.hip), over the lengths the fused kernel does not
  take: {packed, unpacked} x {direct, Rader, Bluestein row}, every templated
  radix (2 / 3 / 4 / 5 / 8) and every radix of the generic stage, each over
  one row and over several rows per workgroup where the plans have both,
  one-point rows, several rows per workgroup and one.

(b) checks hb_div's exactness over the divisors the plans hold, (c) the
constant table HB_CP against cos / sin at 60 digits."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

ND_LO, ND_HI = 16, 20480          # the fused kernel plans nothing above 19,840 (HB_T * HB_RMPER = 20,480 caps per)

# Greedy covers of the branches over ND_LO..ND_HI, cheapest length first
# (tools: `python -m tests.test_hilbert_plan` prints them from the driver).
FUSED_ND = [
    48, 74, 82, 86, 94, 118, 128, 134, 142, 146, 150, 166, 196, 206, 254, 262, 274, 278, 298, 302, 314, 334, 346,
    352, 358, 362, 382, 386, 394, 398, 422, 442, 446, 454, 458, 466, 478, 482, 502, 512, 514, 526, 538, 542, 554,
    562, 566, 586, 614, 622, 626, 634, 646, 662, 674, 694, 698, 706, 718, 734, 746, 758, 766, 778, 794, 802, 1024,
    1102, 1144, 1922, 2048, 2116, 3074, 4096, 4346, 5246, 6912, 7178, 8192, 8366, 9322, 10282, 11520, 12322, 12482,
    13520, 14338, 15478, 15842, 16384, 16498, 17762, 18496, 18734, 18818, 18908, 19610,
]
LONGFFT_ND = [107, 177, 183, 211, 227, 247, 818, 878, 899, 1013, 1517, 1861, 1889, 1901, 1973, 1979, 1999, 2003, 2021]
# rocFFT chirp-z (k_bluestein.hip) takes what neither plans: every odd Nd below
# 64, and Nd whose M has a prime factor the four-step rows cannot hold
BLUESTEIN_ND = [17, 23, 63, 4106, 12101]
# window geometry (other decimations): all fused (2048 k is, up to 16,384)
GEOMETRY_ND = [16, 18, 58, 150, 1024, 2048, 6144, 14336]

# what each swept length runs (plan_label), grouped; test_sweep_plan_is_the_drivers keeps it the driver's
SWEEP_FORMS = {
    "bluestein": [17, 23, 63, 4106, 12101],
    "fused:cp": [18, 48, 58, 150, 196, 352, 442, 646, 1102, 1144, 2116, 6144, 14336],
    "fused:cp+gen": [18734],
    "fused:cp+mf": [3074],
    "fused:gen": [6912, 11520, 13520, 18496],
    "fused:gen+mf": [18908, 19610],
    "fused:mf": [74, 82, 86, 94, 118, 134, 142, 146, 166, 206, 254, 262, 274, 278, 298, 302, 314, 334, 346, 358,
        362, 382, 386, 398, 422, 446, 454, 458, 466, 478, 482, 502, 514, 526, 538, 542, 554, 562, 566, 586, 614,
        622, 626, 634, 662, 674, 694, 698, 706, 718, 734, 746, 758, 766, 778, 794, 802, 1922, 4346, 5246, 7178,
        8366, 9322, 10282, 12322, 12482, 14338, 15478, 15842, 16498, 17762, 18818],
    "fused:r2": [16, 128, 512, 1024, 2048, 4096, 8192, 16384],
    "fused:rd": [394],
    "longfft:bluestein+direct": [227, 878],
    "longfft:direct": [177, 183, 247, 899, 1517, 2021],
    "longfft:direct+rader": [107, 211, 818, 1013, 1861, 1889, 1901, 1973, 1979, 1999, 2003],
}
SWEEP_PLAN = {nd: label for label, nds in SWEEP_FORMS.items() for nd in nds}


def parse(line):
    """One driver line as a dict; stages as (radix, L, form), rows as
    (kind, n, L, rpw, radices)."""
    d = dict(kv.split("=", 1) for kv in line.split())
    out = {k: int(d[k]) for k in ("nd", "fused", "lf", "per", "lds", "pack", "A", "B") if k in d}
    if "stages" in d:
        out["stages"] = [(int(r), int(L), form) for r, L, form in (s.split(":") for s in d["stages"].split(","))]
    for k in ("rowA", "rowB"):
        if k in d:
            kind, n, L, rpw, rad = d[k].split(":")
            out[k] = (kind, int(n), int(L), int(rpw), [int(r) for r in rad.split(".")] if rad else [])
    return out


def fused_branches(p):
    """The fused kernel's plan branches a length runs (empty: not fused)."""
    if not p["fused"]:
        return set()
    b = {("stage", r, form, "L=1" if L == 1 else "L>1") for r, L, form in p["stages"] if r > 2}
    b.add(("radix-2 stages", sum(1 for r, _, _ in p["stages"] if r == 2)))
    b.add(("per", p["per"]))
    return b


LF_TEMPLATED = (2, 3, 4, 5, 8)    # lds_fft's switch (k_longfft.hip); every other radix takes lf_stage_gen


def longfft_branches(p):
    """The four-step DFT's plan branches of a length the fused kernel leaves to it."""
    if p["fused"] or not p["lf"]:
        return set()
    b = set()
    for kind, n, L, rpw, rad in (p["rowA"], p["rowB"]):
        b.add(("row", "packed" if p["pack"] else "unpacked", kind))
        rows = "several rows" if rpw > 1 else "one row"          # per workgroup: the stages' row loop
        b.update(("templated radix" if r in LF_TEMPLATED else "generic radix", r, rows) for r in rad)
        b.add("rpw > 1" if rpw > 1 else "rpw == 1")
        if n == 1:
            b.add("one-point rows")
    return b


def selected(p):
    """The transform the host picks (k_envelope_native.hip, "Hilbert + envelope")."""
    return "fused" if p["fused"] else "longfft" if p["lf"] else "bluestein"


def plan_label(p):
    """What a length runs, as the GPU sweep reports its error: the transform
    and its stage forms / row kinds."""
    if p["fused"]:
        return "fused:" + ("+".join(sorted({form for r, _, form in p["stages"] if r > 2})) or "r2")
    if p["lf"]:
        return "longfft:" + "+".join(sorted({p["rowA"][0], p["rowB"][0]}))
    return "bluestein"


def build_driver(workdir):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(workdir), "hilbert_plan_driver")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-o", exe,
                        os.path.join(HERE, "hilbert_plan_driver.hip")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]

    def run(*cases):
        r = subprocess.run([exe, *[str(c) for c in cases]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def plans_of(run, nds):
    """{Nd: parsed plan} for a list of lengths."""
    plans = [parse(ln) for ln in run(*nds)] if nds else []
    assert [p["nd"] for p in plans] == list(nds)
    return dict(zip(nds, plans))


def greedy_cover(plans, branches, cost):
    """Lengths covering every branch that occurs: repeatedly the length with
    the most uncovered branches per unit of cost; then lengths that the rest
    make redundant are dropped, costliest first."""
    of = {nd: branches(p) for nd, p in plans.items()}
    of = {nd: b for nd, b in of.items() if b}
    todo = set().union(*of.values())
    pick = []
    while todo:
        nd = max(of, key=lambda n: (len(of[n] & todo) / cost(n), -n))
        pick.append(nd)
        todo -= of[nd]
    for nd in sorted(pick, key=cost, reverse=True):
        rest = [n for n in pick if n != nd]
        if set().union(*[of[n] for n in rest]) >= of[nd]:
            pick = rest
    return sorted(pick)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("hilbert_plan"))


@pytest.fixture(scope="module")
def all_plans(driver):
    plans = [parse(ln) for ln in driver(f"{ND_LO}-{ND_HI}")]
    assert [p["nd"] for p in plans] == list(range(ND_LO, ND_HI + 1))
    return {p["nd"]: p for p in plans}


def _union(plans, nds, branches):
    return set().union(*[branches(plans[nd]) for nd in nds])


def test_fused_sweep_covers_every_plan_branch(all_plans):
    """(a) for k_hilbert_env."""
    everything = _union(all_plans, all_plans, fused_branches)
    assert all(all_plans[nd]["fused"] for nd in FUSED_ND)
    assert sorted(set(FUSED_ND)) == FUSED_ND and FUSED_ND[-1] <= ND_HI
    swept = _union(all_plans, FUSED_ND, fused_branches)
    assert swept == everything, sorted(everything - swept, key=str)
    # the enumeration itself: every form, both positions, every count and run length
    assert {b[2] for b in everything if b[0] == "stage"} == {"cp", "mf", "rd", "gen"}
    assert {b[1] for b in everything if b[0] == "radix-2 stages"} == set(range(14))
    assert {b[1] for b in everything if b[0] == "per"} == set(range(1, 21))
    # nothing in the list is idle: every length is the only one with some branch
    for nd in FUSED_ND:
        assert _union(all_plans, [n for n in FUSED_ND if n != nd], fused_branches) != everything, nd


def test_longfft_sweep_covers_every_plan_branch(all_plans):
    """(a) for k_longfft.hip, over the lengths the fused kernel does not take."""
    everything = _union(all_plans, all_plans, longfft_branches)
    assert all(selected(all_plans[nd]) == "longfft" for nd in LONGFFT_ND)
    assert sorted(set(LONGFFT_ND)) == LONGFFT_ND and LONGFFT_ND[-1] < 5000
    swept = _union(all_plans, LONGFFT_ND, longfft_branches)
    assert swept == everything, sorted(everything - swept, key=str)
    assert {b for b in everything if b[0] == "row"} == {("row", pk, kind) for pk in ("packed", "unpacked")
                                                        for kind in ("direct", "rader", "bluestein")}
    assert {b[1:] for b in everything if b[0] == "templated radix"} == {(r, rows) for r in LF_TEMPLATED
                                                                        for rows in ("one row", "several rows")}
    primes = [p for p in range(7, 62) if all(p % q for q in range(2, p))]
    assert {b[1] for b in everything if b[0] == "generic radix"} == set(primes)
    assert {"one-point rows", "rpw > 1", "rpw == 1"} <= everything
    for nd in LONGFFT_ND:
        assert _union(all_plans, [n for n in LONGFFT_ND if n != nd], longfft_branches) != everything, nd


def test_sweep_plan_is_the_drivers(all_plans):
    """SWEEP_PLAN, from which the GPU sweep knows which kernels to expect in
    the profile, is what the driver says of every swept length."""
    nds = sorted(set(FUSED_ND + LONGFFT_ND + BLUESTEIN_ND + GEOMETRY_ND))
    assert SWEEP_PLAN == {nd: plan_label(all_plans[nd]) for nd in nds}
    assert all(SWEEP_PLAN[nd] == "bluestein" for nd in BLUESTEIN_ND)
    assert all(SWEEP_PLAN[nd].startswith("fused:") for nd in GEOMETRY_ND)
    assert {17, 19, 61, 63} <= {nd for nd, p in all_plans.items() if selected(p) == "bluestein"}


def test_selection_limits(all_plans):
    """The limits the two plans state: the fused kernel takes even Nd up to
    19,840 whose half factors into primes <= 401 (and fits LDS and the
    threads' budget); the four-step DFT nothing below 64."""
    fused = [nd for nd, p in all_plans.items() if p["fused"]]
    assert max(fused) == 19840 and not any(nd % 2 for nd in fused)
    for nd in fused:
        p = all_plans[nd]
        assert max(r for r, _, _ in p["stages"]) <= 401 and p["lds"] <= 160 * 1024
        assert p["per"] == -(-nd // 1024)
        m = nd // 2
        for r, L, _ in p["stages"]:
            m //= r
            assert L == m
        assert m == 1
    assert not any(p["lf"] for nd, p in all_plans.items() if nd < 64)
    assert all_plans[2018]["rowB"][1] == 1                    # M = 1009, a prime > 64: B == 1


def test_magic_division_is_exact(driver):
    """(b) hb_div(x, hb_magic(d)) == x / d for every divisor the plans hold
    (dL, dP, dH, dG, dT; the driver also checks that each multiplier is
    hb_magic of its divisor) and every 0 <= x < 16 * 16384, the header's
    bound on the kernel's dividends (16 M, M < 16384)."""
    (line,) = driver(f"magic:{ND_LO}-{ND_HI}")
    d = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
    assert d["bad"] == 0
    assert d["divisors"] > 2000 and d["checked"] == d["divisors"] * 16 * 16384
    assert d["max"] * 16 * 16384 < 2 ** 32                    # x d < 2^32, the header's condition


def test_constant_table_is_correctly_rounded(driver):
    """(c) every HB_CP entry, read back through hb_radixp_const's addressing,
    is cos / sin (2 pi n k / p) correctly rounded, and hb_cp_off agrees with
    the layout (the driver fails on a wrong offset or non-zero padding)."""
    lines = driver("cp")
    offs = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("off ")]
    assert [p for p, _, _ in offs] == [3, 5, 7, 11, 13, 17, 19, 23, 29]
    size = [ln for ln in lines if ln.startswith("size ")]
    assert len(size) == 1 and size[0].split()[1] == size[0].split()[2]
    o = 0
    for p, off, ng in offs:                                   # per prime: ng groups of (p - 1) / 2 rows of 2 x 6
        assert off == o and ng == -(-((p + 1) // 2) // 6)
        o += ng * ((p - 1) // 2) * 12
    assert o == int(size[0].split()[1])
    entries = [ln.split() for ln in lines if ln[0].isdigit()]
    assert len(entries) == sum(((p - 1) // 2) * ((p + 1) // 2) for p, _, _ in offs)
    assert len({tuple(e[:3]) for e in entries}) == len(entries)
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    for p, n, k, c, s in entries:
        a = 2 * mp.pi * int(n) * int(k) / int(p)
        assert float(c) == float(mp.cos(a)), (p, n, k, "cos")
        assert float(s) == float(mp.sin(a)), (p, n, k, "sin")


if __name__ == "__main__":                                    # regenerate the two lists
    import tempfile
    run = build_driver(tempfile.mkdtemp())
    plans = {p["nd"]: p for p in map(parse, run(f"{ND_LO}-{ND_HI}"))}
    f = greedy_cover(plans, fused_branches, lambda nd: nd + 2000)
    print("FUSED_ND =", f, len(f), sum(f), len(_union(plans, f, fused_branches)))
    lf = greedy_cover({nd: p for nd, p in plans.items() if nd < 5000}, longfft_branches, lambda nd: nd + 2000)
    print("LONGFFT_ND =", lf, len(lf), sum(lf), len(_union(plans, lf, longfft_branches)))
    forms = {}
    for nd in sorted(set(f + lf + BLUESTEIN_ND + GEOMETRY_ND)):
        forms.setdefault(plan_label(plans[nd]), []).append(nd)
    print("SWEEP_FORMS =", dict(sorted(forms.items())))
