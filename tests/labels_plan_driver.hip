/*
 * labels_plan_driver.hip — prints labels_plan (csrc/bpmx_plan.h) for
 * tests/test_labels_abi.py.  Host code only: it runs without a GPU.
 *
 * Each argument F:cap_peaks:options gives one line of key=value pairs; the
 * first line holds the structure sizes of include/bpmx.h.
 */
#include <cstdio>
#include <cstdlib>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_out=%zu threads=%d record=%d per=%d\n", sizeof(bpmx_label_params),
                sizeof(bpmx_labels_out), (int)LABELS_T, (int)BPMX_LABELS_RECORD, (int)LB_PER);
    for (int i = 1; i < argc; ++i) {
        long long F = 0, cap = 0, opt = 0;
        if (std::sscanf(argv[i], "%lld:%lld:%lld", &F, &cap, &opt) != 3) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const LabelsPlan L = labels_plan((int)F, cap, (int32_t)opt);
        std::printf("grid=%u lds_n=%lld lds=%zu any_global=%d fixed=%zu gws=%zu budget=%zu max_n=%lld bytes_605=%zu "
                    "stride=%d\n",
                    L.grid, (long long)L.lds_n, L.lds, (int)L.any_global, L.fixed, L.gws, LABELS_LDS_BUDGET,
                    (long long)labels_ws_max_n(LABELS_LDS_BUDGET, LABELS_T), labels_ws_bytes(605, LABELS_T),
                    (int)LB_STRIDE);
    }
    return 0;
}
