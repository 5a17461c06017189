/*
 * marks_plan_driver.hip — prints marks_plan (csrc/bpmx_plan.h) for
 * tests/test_marks_abi.py.  Host code only: it runs without a GPU.
 *
 * Each argument F:cap_ref:options gives one line of key=value pairs; the first
 * line holds the structure sizes of include/bpmx.h.
 */
#include <cstdio>
#include <cstdlib>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_ref=%zu sizeof_packed=%zu sizeof_beats=%zu threads=%d record=%d per_s1=%d "
                "stride=%d scratch=%d per_file=%d\n",
                sizeof(bpmx_marks_params), sizeof(bpmx_ref_marks), sizeof(bpmx_packed), sizeof(bpmx_beats_out),
                (int)MARKS_T, (int)BPMX_MARKS_RECORD, (int)BEATS_WS_PER_PEAK, (int)MK_STRIDE, (int)MK_SCRATCH,
                (int)MC_PER_FILE);
    for (int i = 1; i < argc; ++i) {
        long long F = 0, ref = 0, opt = 0;
        if (std::sscanf(argv[i], "%lld:%lld:%lld", &F, &ref, &opt) != 3) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const MarksPlan M = marks_plan((int)F, ref, (int32_t)opt);
        std::printf("grid=%u lds_n=%lld lds=%zu any_global=%d fixed=%zu gws=%zu rows=%zu o_ridx=%zu o_ktype=%zu "
                    "o_rtag=%zu o_cnt=%zu budget=%zu max_n=%lld bytes=%zu head=%zu\n",
                    M.grid, (long long)M.lds_n, M.lds, (int)M.any_global, M.fixed, M.gws, M.rows, M.o_ridx, M.o_ktype,
                    M.o_rtag, M.o_cnt, MARKS_LDS_BUDGET, (long long)marks_ws_max_n(MARKS_LDS_BUDGET, MARKS_T),
                    marks_ws_bytes(ref, MARKS_T), marks_ws_head(MARKS_T));
    }
    return 0;
}
