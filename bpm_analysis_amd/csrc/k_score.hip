/*
 * k_score.hip — bpmx_score_device: the label rows of k_labels scored against
 * a person's corrected marks (TP, SWAP, FP, FN per type, the timing errors of
 * the TP, the per-mark rows), one workgroup of SCORE_T threads per recording.
 *
 * The logic is bpmx_score_core.h, the same text the host tests run; this file
 * gives it the workgroup executor and the memory.  Parallel: the millisecond
 * conversions, the span heads and their compaction, the span lookup of every
 * label row, the compactions by type, the row outputs.  The two walks of a
 * pass share no list: threads 0 and 1 run them side by side between two
 * barriers, then the two walks of the next pass.
 *
 * Memory: a recording whose workspace is at most A.lds bytes keeps it in LDS
 * (bpmx_plan.h: 32 KB, five workgroups per CU).  A longer one works in its
 * slice of the global buffer.  The label rows and the reference marks are
 * read where they lie.  It reads pk_off, rf_off, n_labels and the labels
 * status itself, so nothing synchronises the host.  Nothing is read or
 * written beyond the capacities: a recording whose slice reaches past one
 * only reports BPMX_SCORE_OVERFLOW.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_score_core.h"

namespace bpmx {

namespace {
struct score_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return SCORE_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(SCORE_T) void k_score(ScoreArgs A) {
    extern __shared__ __align__(16) unsigned char score_lds[];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t o = A.pk_off[f], e = A.pk_off[f + 1], n = e - o;
    const int64_t ro = A.rf_off[f], re = A.rf_off[f + 1], nr = re - ro;
    if (o < 0 || n < 0 || e > A.cap || ro < 0 || nr < 0 || re > A.cap_ref) {
        if (lane == 0) A.O.status[f] = BPMX_SCORE_OVERFLOW;
        return;
    }
    /* a labels status other than OK, or a count its slice cannot hold: no detected marks */
    int64_t nd = A.n_labels[f];
    const bool labelled = A.l_status[f] == BPMX_LABELS_OK && nd >= 0 && nd <= n;
    if (!labelled) nd = 0;
    const bool in_lds = score_ws_bytes(nd, nr, SCORE_T) <= A.lds;
    void *base = in_lds ? (void *)score_lds : (void *)(A.gws + (size_t)f * A.fixed + (size_t)(o + ro) * SC_STRIDE);
    const score_ws w = score_ws_layout(base, nd, nr, SCORE_T);
    score_io io;
    const bool rows = A.O.sc_kind != nullptr;
    io.sc_kind = rows ? A.O.sc_kind + o : nullptr; io.sc_ref = rows ? A.O.sc_ref + o : nullptr;
    io.rf_kind = rows ? A.O.rf_kind + ro : nullptr; io.rf_det = rows ? A.O.rf_det + ro : nullptr;
    io.record = A.O.record + (size_t)f * BPMX_SCORE_RECORD;
    const int rc = score_core(score_group(), nd, A.lb_time + o, A.lb_type + o, nr, A.rf_ms + ro, A.rf_type + ro, A.P,
                              w, io);
    if (lane == 0) A.O.status[f] = rc == BPMX_SCORE_OK && !labelled ? BPMX_SCORE_NO_LABELS : rc;
}

}  // namespace bpmx
