/*
 * metrics_plan_driver.hip — prints metrics_plan (csrc/bpmx_plan.h) for
 * tests/test_metrics_abi.py.  Host code only: it runs without a GPU.
 *
 * Each argument F:cap_peaks:options:hrv_window gives one line of key=value
 * pairs; the first line holds the structure sizes of include/bpmx.h.
 */
#include <cstdio>
#include <cstdlib>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_out=%zu sizeof_frame=%zu threads=%d record=%d\n", sizeof(bpmx_metric_params),
                sizeof(bpmx_metrics_out), sizeof(pw_frame), (int)METRICS_T, (int)BPMX_METRICS_RECORD);
    for (int i = 1; i < argc; ++i) {
        long long F = 0, cap = 0, opt = 0, win = 0;
        if (std::sscanf(argv[i], "%lld:%lld:%lld:%lld", &F, &cap, &opt, &win) != 4) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const MetricsPlan M = metrics_plan((int)F, cap, (int32_t)opt, (int32_t)win);
        std::printf("grid=%u fw=%d lds_n=%lld lds=%zu any_global=%d fixed=%zu gws=%zu budget=%zu max_n=%lld "
                    "bytes_605=%zu stride=%d\n",
                    M.grid, M.fw, (long long)M.lds_n, M.lds, (int)M.any_global, M.fixed, M.gws, METRICS_LDS_BUDGET,
                    (long long)metrics_ws_max_n(METRICS_LDS_BUDGET, METRICS_T, M.fw),
                    metrics_ws_bytes(605, METRICS_T, M.fw, true), (int)MX_STRIDE);
    }
    return 0;
}
