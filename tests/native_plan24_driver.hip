/*
 * native_plan24_driver.hip — prints native mode's block-kernel plan
 * (csrc/bpmx_native_plan.h: native_block_plan) with the packed 24-bit format
 * and its two matrix-core routes, for tests/test_native_plan24.py.  Host code
 * only: it runs without a GPU.  The line format is native_plan_driver.hip's.
 *
 * Arguments:
 *   <dtype>:<channels>:<ds>:<options>:<align>:<total>
 *        dtype u8 i16 i32 f32 f64 i24; align the PCM address mod 16; total the
 *        batch's elements.  One line of key=value pairs:
 *        rc route [gen=<dtype>:<mono|multi>:<staged|direct>] bt gstr lds ndma mfma_ks big_ks big_bs key15 key16
 *        (rc=-3 alone beyond NAT_DSMAX)
 *   rec:<ds>:<bt>:<n>   a recording of n frames in tiles of bt blocks:
 *        nd nb tf lp nt tail=<par|serial> scan=<reg|chunked>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_native_plan.h"

using namespace bpmx;

static const char *const DTYPES[] = {"u8", "i16", "i32", "f32", "f64", "i24"};
static const char *const ROUTES[] = {"mfma<3>", "mfma<5>", "big<5>", "big<10>", "dma<1>",
                                     "dma<2>",  "i16",     "gen",    "mfma24<3>", "mfma24<5>"};
static_assert(NAT_R_M24_5 == 9 && NAT_R_GEN == 7 && BPMX_DT_I24 == 5, "the tables above");

static int bad(const char *a) {
    std::fprintf(stderr, "bad case: %s\n", a);
    return 2;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        if (std::strncmp(a, "rec:", 4) == 0) {
            long long ds = 0, bt = 0, n = 0;
            if (std::sscanf(a + 4, "%lld:%lld:%lld", &ds, &bt, &n) != 3 || ds < 1 || bt < 1 || n < 1) return bad(a);
            const long long nd = (n + ds - 1) / ds, nb = nd - 1, tf = nb / bt;
            std::printf("nd=%lld nb=%lld tf=%lld lp=%lld nt=%lld tail=%s scan=%s\n", nd, nb, tf, nb - tf * bt,
                        (long long)nat_tail_len(n, (int)ds), nat_tail_parallel(n, (int)ds) ? "par" : "serial",
                        nat_carry_chunked(n, (int)ds, (int)bt) ? "chunked" : "reg");
            continue;
        }
        char dt[8] = {0};
        long long ch = 0, ds = 0, opt = 0, align = 0, total = 0;
        if (std::sscanf(a, "%7[^:]:%lld:%lld:%lld:%lld:%lld", dt, &ch, &ds, &opt, &align, &total) != 6) return bad(a);
        int dtype = -1;
        for (int k = 0; k < 6; ++k)
            if (std::strcmp(dt, DTYPES[k]) == 0) dtype = k;
        if (dtype < 0 || ch < 1 || ds < 1 || align < 0 || align > 15 || total < 0) return bad(a);
        NativePlan P;
        const int rc = native_block_plan(dtype, (int)ch, (int)ds, (int32_t)opt, (unsigned)align, total, &P);
        std::printf("rc=%d", rc);
        if (rc == BPMX_OK) {
            std::printf(" route=%s", ROUTES[P.route]);
            if (P.route == NAT_R_GEN)
                std::printf(" gen=%s:%s:%s", DTYPES[P.gen_dtype], P.gen_multi ? "multi" : "mono",
                            P.gen_staged ? "staged" : "direct");
            std::printf(" bt=%d gstr=%lld lds=%zu ndma=%d mfma_ks=%d big_ks=%d big_bs=%d key15=%lld key16=%lld", P.bt,
                        (long long)P.gstr, P.lds, P.ndma, P.mfma_ks, P.big_ks, P.big_bs, (long long)P.key15,
                        (long long)P.key16);
        }
        std::printf("\n");
    }
    return 0;
}
