/*
 * native_plan_driver.hip — prints native mode's block-kernel plan
 * (csrc/bpmx_native_plan.h: native_block_plan, nat_tail_parallel,
 * nat_carry_chunked) for tests/test_native_plan.py.  Host code only: it runs
 * without a GPU.
 *
 * Arguments:
 *   <dtype>:<channels>:<ds>:<options>:<align>:<total>
 *        dtype u8 i16 i32 f32 f64; align the PCM address mod 16; total the
 *        batch's elements.  One line of key=value pairs:
 *        rc route [gen=<dtype>:<mono|multi>:<staged|direct>] bt gstr lds ndma mfma_ks big_ks big_bs key15 key16
 *        (rc=-3 alone beyond NAT_DSMAX)
 *   rec:<ds>:<bt>:<n>   a recording of n frames in tiles of bt blocks:
 *        nd nb tf lp nt tail=<par|serial> scan=<reg|chunked>
 *   all:<lo>-<hi>      every plan of ds in [lo, hi] x dtype x 1..3 channels x the
 *        two native options x every element-aligned address: the distinct
 *        routes (gen with its instantiation) and tile-length classes
 *        (bt=64, bt:even, bt:odd), one "name count" line each
 *   limits             dsmax tt_par cpf
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../bpm_analysis_amd/csrc/bpmx_native_plan.h"

using namespace bpmx;

static const char *const DTYPES[] = {"u8", "i16", "i32", "f32", "f64"};
static const char *const ROUTES[] = {"mfma<3>", "mfma<5>", "big<5>", "big<10>", "dma<1>", "dma<2>", "i16", "gen"};

static int bad(const char *a) {
    std::fprintf(stderr, "bad case: %s\n", a);
    return 2;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        if (std::strcmp(a, "limits") == 0) {
            std::printf("dsmax=%d tt_par=%d cpf=%d\n", NAT_DSMAX, NAT_TT_PAR, NAT_CPF);
            continue;
        }
        if (std::strncmp(a, "all:", 4) == 0) {
            long long lo = 0, hi = 0;
            if (std::sscanf(a + 4, "%lld-%lld", &lo, &hi) != 2 || lo < 1 || hi < lo) return bad(a);
            std::map<std::string, long long> seen;
            static const int opts[] = {0, BPMX_OPT_NATIVE_F64, BPMX_OPT_NATIVE_DMA, BPMX_OPT_NATIVE_F64 | BPMX_OPT_NATIVE_DMA};
            for (int dtype = 0; dtype < 5; ++dtype)
                for (int ch = 1; ch <= 3; ++ch)
                    for (long long ds = lo; ds <= hi; ++ds)
                        for (int opt : opts)
                            for (unsigned align = 0; align < 16; ++align) {
                                if (align % (dtype == BPMX_DT_U8 ? 1 : dtype == BPMX_DT_I16 ? 2 : dtype == BPMX_DT_F64 ? 8 : 4))
                                    continue;                    /* PCM is aligned to its element */
                                NativePlan P;
                                if (native_block_plan(dtype, ch, (int)ds, opt, align, 1 << 20, &P) != BPMX_OK) {
                                    ++seen["limit"];
                                    continue;
                                }
                                std::string k = ROUTES[P.route];
                                if (P.route == NAT_R_GEN)
                                    k += std::string(":") + DTYPES[P.gen_dtype] + (P.gen_multi ? ":multi" : ":mono") +
                                         (P.gen_staged ? ":staged" : ":direct");
                                ++seen[k];
                                ++seen[P.bt == 64 ? "bt=64" : P.bt % 2 ? "bt:odd" : "bt:even"];
                                if (P.bt < 1 || P.bt > 64) ++seen["bt:out-of-range"];
                            }
            for (const auto &kv : seen) std::printf("%s %lld\n", kv.first.c_str(), kv.second);
            continue;
        }
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
        for (int k = 0; k < 5; ++k)
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
