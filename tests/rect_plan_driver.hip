/*
 * rect_plan_driver.hip — prints rect_plan (csrc/bpmx_plan.h) for
 * tests/test_rect_plan.py.  Host code only: it runs without a GPU.
 *
 * Each argument is one case and gives one line of key=value pairs:
 *   rect:dtype:channels:window:options:F:maxn
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        long long v[6] = {};
        int n = 0;
        char *p = std::strchr(argv[i], ':');
        while (p && n < 6) {
            v[n++] = std::strtoll(p + 1, &p, 10);
            if (*p != ':') p = nullptr;
        }
        if (std::strncmp(argv[i], "rect:", 5) != 0 || n != 6) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const RectPlan R = rect_plan((int)v[0], (int)v[1], v[2], (int32_t)v[3], (int)v[4], v[5]);
        static const char *const route[] = {"int_lds", "int_global", "general"};
        std::printf("route=%s integer=%d chunk=%lld nch=%lld lds=%zu csum_bytes=%zu rows_bytes=%zu grid=%u,%u"
                    " g_pick=%u,%u g_seq=%u w_exact_max=%lld lds_n=%lld threads=%d\n",
                    route[R.route], R.integer, (long long)R.chunk, (long long)R.nch, R.lds, R.csum_bytes, R.rows_bytes,
                    R.grid.x, R.grid.y, R.g_pick.x, R.g_pick.y, R.g_seq.x, (long long)RECT_W_EXACT_MAX,
                    (long long)RECT_LDS_N, RECT_T);
    }
    return 0;
}
