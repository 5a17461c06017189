/*
 * beats_plan_driver.hip — prints beats_plan (csrc/bpmx_plan.h) for
 * tests/test_beats_abi.py.  Host code only: it runs without a GPU.
 *
 * Each argument F:cap_peaks:options gives one line of key=value pairs.
 */
#include <cstdio>
#include <cstdlib>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        long long F = 0, cap = 0, opt = 0;
        if (std::sscanf(argv[i], "%lld:%lld:%lld", &F, &cap, &opt) != 3) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const BeatsPlan B = beats_plan((int)F, cap, (int32_t)opt);
        std::printf("grid=%u lds_n=%lld lds=%zu any_global=%d gws=%zu budget=%zu max_peaks=%lld bytes_605=%zu "
                    "fixed=%d stride=%d\n",
                    B.grid, (long long)B.lds_n, B.lds, (int)B.any_global, B.gws, BEATS_LDS_BUDGET,
                    (long long)beats_ws_max_peaks(BEATS_LDS_BUDGET), beats_ws_bytes(605, true), (int)BEATS_WS_FIXED,
                    (int)BEATS_WS_STRIDE);
    }
    return 0;
}
