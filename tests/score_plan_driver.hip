/*
 * score_plan_driver.hip — prints score_plan (csrc/bpmx_plan.h) for
 * tests/test_score_abi.py.  Host code only: it runs without a GPU.
 *
 * Each argument F:cap_peaks:cap_ref:options gives one line of key=value
 * pairs; the first line holds the structure sizes of include/bpmx.h.
 */
#include <cstdio>
#include <cstdlib>

#include "../bpm_analysis_amd/csrc/bpmx_plan.h"

using namespace bpmx;

int main(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_ref=%zu sizeof_out=%zu threads=%d record=%d per_det=%d per_ref=%d stride=%d\n",
                sizeof(bpmx_score_params), sizeof(bpmx_ref_marks), sizeof(bpmx_score_out), (int)SCORE_T,
                (int)BPMX_SCORE_RECORD, (int)SC_PER_DET, (int)SC_PER_REF, (int)SC_STRIDE);
    for (int i = 1; i < argc; ++i) {
        long long F = 0, cap = 0, ref = 0, opt = 0;
        if (std::sscanf(argv[i], "%lld:%lld:%lld:%lld", &F, &cap, &ref, &opt) != 4) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const ScorePlan S = score_plan((int)F, cap, ref, (int32_t)opt);
        std::printf("grid=%u lds=%zu any_global=%d fixed=%zu gws=%zu budget=%zu max_n=%lld bytes=%zu head=%zu\n", S.grid,
                    S.lds, (int)S.any_global, S.fixed, S.gws, SCORE_LDS_BUDGET,
                    (long long)score_ws_max_n(SCORE_LDS_BUDGET, SCORE_T), score_ws_bytes(cap, ref, SCORE_T),
                    score_ws_head(SCORE_T));
    }
    return 0;
}
