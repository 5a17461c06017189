/*
 * hilbert_plan_driver.hip — prints the plans of the device Hilbert transforms
 * (csrc/k_hilbert.hip: hilbert_plan; csrc/k_longfft.hip: longfft_supported,
 * lf_shape, lf_sub_shape) for tests/test_hilbert_plan.py.  Host code only: it
 * runs without a GPU.
 *
 * Arguments:
 *   <Nd> | <lo>-<hi>   one line of key=value pairs per decimated length:
 *        nd fused [per lds stages=radix:L:form,...]   form: r2 cp mf rd gen
 *        lf [pack A B rowA= rowB=]   row: kind:n:L:rpw:radix.radix...  kind: direct rader bluestein
 *   magic:<lo>-<hi>    hb_div(x, hb_magic(d)) == x / d for every divisor d the
 *        fused plans of these lengths hold and every 0 <= x < 16 * 16384
 *        (hilbert_plan refuses M >= 16384); prints divisors= checked= bad=
 *   cp                 HB_CP as "p n k cos sin" lines (17 significant digits),
 *        zero padding checked here; then "off p offset groups" per prime
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../bpm_analysis_amd/csrc/k_hilbert.hip"
#define cmul lf_cmul          /* both files define one (the library compiles them apart) */
#include "../bpm_analysis_amd/csrc/k_longfft.hip"
#undef cmul

/* the host has no copy of a __constant__ array's values: the table's text once
 * more as a host array */
#undef BPMX_DFT_CONSTS_H
#pragma push_macro("__constant__")
#undef __constant__
#define __constant__ static const
#define bpmx hb_host_copy
#include "../bpm_analysis_amd/csrc/bpmx_dft_consts.h"
#undef bpmx
#pragma pop_macro("__constant__")

int bpmx::fail(int code, const std::string &msg) {
    std::fprintf(stderr, "bpmx::fail(%d): %s\n", code, msg.c_str());
    return code;
}

using namespace bpmx;

static void print_row(const char *name, int32_t n) {
    static const char *const kinds[] = {"direct", "bluestein", "rader"};
    const LfSub sb = lf_sub_shape(n);
    std::printf(" %s=%s:%d:%d:%d:", name, kinds[sb.kind], sb.n, sb.L, sb.rpw);
    for (int i = 0; i < sb.nrad; ++i) std::printf("%s%d", i ? "." : "", sb.rad[i]);
}

static void plan_line(int64_t nd) {
    HilbPlan P;
    std::vector<double2> tabs;
    size_t lds = 0;
    /* the host's own condition (k_envelope_native.hip): nd > 15, then the plan */
    const int fused = nd > 15 && hilbert_plan(nd, 30, &P, &tabs, &lds);
    std::printf("nd=%lld fused=%d", (long long)nd, fused);
    if (fused) {
        std::printf(" per=%d lds=%zu stages=", P.per, lds);
        for (int i = 0; i < P.ns; ++i) {
            const char *form = P.rad[i] == 2 ? "r2" : P.cp[i] ? "cp" : P.rd[i] ? "rd" : P.mf[i] ? "mf" : "gen";
            std::printf("%s%d:%d:%s", i ? "," : "", P.rad[i], P.L[i], form);
        }
    }
    const int lf = longfft_supported(nd);
    std::printf(" lf=%d", lf);
    if (lf) {
        const int pack = nd % 2 == 0;
        int32_t A = 0, B = 0;
        lf_shape(pack ? nd / 2 : nd, &A, &B);
        std::printf(" pack=%d A=%d B=%d", pack, A, B);
        print_row("rowA", A);
        print_row("rowB", B);
    }
    std::printf("\n");
}

static int magic_check(int64_t lo, int64_t hi) {
    std::set<uint32_t> divs;
    for (int64_t nd = lo; nd <= hi; ++nd) {
        HilbPlan P;
        std::vector<double2> tabs;
        size_t lds = 0;
        if (!hilbert_plan(nd, 30, &P, &tabs, &lds)) continue;
        for (int i = 0; i < P.ns; ++i) {
            const int r = P.rad[i], h = (r - 1) / 2;
            const uint32_t d[5] = {(uint32_t)P.L[i], (uint32_t)r, (uint32_t)(h > 0 ? h : 1),
                                   (uint32_t)((h + HB_KB) / HB_KB), (uint32_t)((h + 16) / 16)};
            const uint64_t m[5] = {P.dL[i], P.dP[i], P.dH[i], P.dG[i], P.dT[i]};
            for (int j = 0; j < 5; ++j) {
                if (m[j] != hb_magic(d[j])) {
                    std::printf("plan nd=%lld stage %d: multiplier %d is not hb_magic(%u)\n", (long long)nd, i, j, d[j]);
                    return 1;
                }
                divs.insert(d[j]);
            }
        }
    }
    long long checked = 0, bad = 0;
    for (uint32_t d : divs) {
        const uint64_t m = hb_magic(d);
        uint32_t q = 0, r = 0;
        for (int x = 0; x < 16 * 16384; ++x) {
            bad += (uint32_t)hb_div(x, m) != q;
            if (++r == d) { r = 0; ++q; }
        }
        checked += 16 * 16384;
    }
    std::printf("divisors=%zu max=%u checked=%lld bad=%lld\n", divs.size(), divs.empty() ? 0u : *divs.rbegin(), checked, bad);
    return 0;
}

static int cp_dump() {
    namespace H = hb_host_copy;
    const int G = H::HB_CP_G;
    const int n_tab = (int)(sizeof(H::HB_CP) / sizeof(H::HB_CP[0]));
    int o = 0;
    for (int p = 3; p <= HB_PMAX; p += 2) {
        if (hb_cp_off(p) < 0) continue;
        const int h = (p - 1) / 2, ng = hb_cp_ng(p);
        std::printf("off %d %d %d\n", p, hb_cp_off(p), ng);
        if (hb_cp_off(p) != o || hb_cp_off(p) != H::hb_cp_off(p) || o + ng * h * 2 * G > n_tab) {
            std::printf("layout p=%d: offset %d, rows end at %d of %d\n", p, o, o + ng * h * 2 * G, n_tab);
            return 1;
        }
        /* hb_radixp_const's addressing: row = HB_CP + cpo + g (h 2 G) + (n - 1) 2 G; cos [G] | sin [G] */
        for (int g = 0; g < ng; ++g)
            for (int n = 1; n <= h; ++n) {
                const double *row = H::HB_CP + o + g * (h * 2 * G) + (n - 1) * 2 * G;
                for (int j = 0; j < G; ++j) {
                    const int k = g * G + j;
                    if (k <= h) std::printf("%d %d %d %.17g %.17g\n", p, n, k, row[j], row[G + j]);
                    else if (row[j] != 0.0 || row[G + j] != 0.0) {
                        std::printf("padding p=%d n=%d k=%d is not zero\n", p, n, k);
                        return 1;
                    }
                }
            }
        o += ng * h * 2 * G;
    }
    std::printf("size %d %d\n", o, n_tab);
    return 0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        if (std::strcmp(a, "cp") == 0) {
            if (cp_dump()) return 1;
            continue;
        }
        const bool magic = std::strncmp(a, "magic:", 6) == 0;
        char *e = nullptr;
        const long long lo = std::strtoll(magic ? a + 6 : a, &e, 10);
        const long long hi = *e == '-' ? std::strtoll(e + 1, &e, 10) : lo;
        if (*e || lo < 1 || hi < lo) {
            std::fprintf(stderr, "bad case: %s\n", a);
            return 2;
        }
        if (magic) {
            if (magic_check(lo, hi)) return 1;
        } else {
            for (long long nd = lo; nd <= hi; ++nd) plan_line(nd);
        }
    }
    return 0;
}
