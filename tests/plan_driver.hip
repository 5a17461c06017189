/*
 * plan_driver.hip — prints the launch plans of csrc/bpmx_plan.h for
 * tests/test_plan.py.  Host code only: it runs without a GPU.
 *
 * Each argument is one case and gives one line of key=value pairs:
 *   detect:F:Nd:W:options:ordered:min_periods:distance:stages
 *   ref:Nd:env_window:options
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

static int detect_case(const long long *v) {
    bpmx_params P{};
    const int F = (int)v[0];
    const int64_t nd = v[1];
    P.noise_window = (int32_t)v[2];
    P.options = (int32_t)v[3];
    const bool ordered = v[4] != 0;
    P.min_periods = (int32_t)v[5];
    P.distance = (int32_t)v[6];
    P.stages = (int32_t)v[7];
    DetectPlan D;
    const int rc = detect_plan(P, F, nd, ordered, &D);
    std::printf("rc=%d", rc);
    if (rc != BPMX_OK) {
        std::printf(" lds_g=%zu err=%s\n", D.lds_g, D.err);
        return 0;
    }
    static const char *const rq[] = {"256,16", "256,32", "g"};
    std::printf(" bad_window=%d W=%lld cap=%d lds=%zu long_files=%d fp_global=%d fp_long=%d bounds=%d floor_wm=%d"
                " use_wm=%d need_merge=%d merge_g=%d gcap=%lld lds_g=%zu wm_n=%lld wm_lds_p=%zu wm_lds=%zu"
                " wm_c=%lld wm_chunks=%d wm_nch=%lld chunk=%lld nch=%lld union=%s",
                D.bad_window, (long long)D.W, D.cap, D.lds, D.long_files, D.fp_global, D.fp_long, D.bounds,
                D.floor_wm, D.use_wm, D.need_merge, D.merge_g, (long long)D.gcap, D.lds_g, (long long)D.wm_n,
                D.wm_lds_p, D.wm_lds, (long long)D.wm_c, D.wm_chunks, (long long)D.wm_nch, (long long)D.chunk,
                (long long)D.nch, D.need_merge ? rq[D.rq_union] : "none");
    std::printf(" g2=%u,%u g_unit=%u,%u g_prom=%u,%u g_dch=%u,%u gf=%u,%u gi=%u,%u bs_gy=%u db_gy=%u dp_gy=%u fp_nu=%d\n",
                D.g2.x, D.g2.y, D.g_unit.x, D.g_unit.y, D.g_prom.x, D.g_prom.y, D.g_dch.x, D.g_dch.y, D.gf.x, D.gf.y,
                D.gi.x, D.gi.y, D.bs_gy, D.db_gy, D.dp_gy, D.fp_nu);
    return 0;
}

static int ref_case(const long long *v) {
    const RefEnvPlan R = ref_env_plan(v[0], (int32_t)v[1], (int32_t)v[2]);
    std::printf("chain=%d rows=%lld nfc=%lld wants_split=%d nkc=%d fwd=", R.chain, (long long)R.rows,
                (long long)R.nfc, R.wants_split, R.nkc);
    for (int64_t k = 0; k <= R.nfc; ++k) std::printf("%s%lld", k ? "," : "", (long long)R.fwd_row(k));
    std::printf(" kend=");
    for (int k = 0; k < R.nkc; ++k) std::printf("%s%lld", k ? "," : "", (long long)R.kend[k]);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        long long v[8] = {};
        int n = 0;
        char *p = std::strchr(argv[i], ':');
        while (p && n < 8) {
            v[n++] = std::strtoll(p + 1, &p, 10);
            if (*p != ':') p = nullptr;
        }
        const bool det = std::strncmp(argv[i], "detect:", 7) == 0 && n == 8;
        const bool ref = std::strncmp(argv[i], "ref:", 4) == 0 && n == 3;
        if (!det && !ref) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        if (det ? detect_case(v) : ref_case(v)) return 1;
    }
    return 0;
}
