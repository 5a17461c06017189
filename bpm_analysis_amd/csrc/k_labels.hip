/*
 * k_labels.hip — bpmx_labels_device: the labeler's output (the S1 / S2 label
 * table, the S1->S2 pairs, the groups of marks and their statistics, the
 * per-file mean interval) from k_beats_trace's outputs where they lie, one
 * workgroup of LABELS_T threads per recording.
 *
 * The logic is bpmx_labels_core.h, the same text the host tests run; this
 * file gives it the workgroup executor and the memory.  Parallel: the final
 * type of every raw peak, the compactions, the decimal roundings, the nearest
 * curve row of every label, one group's statistics per thread.  Serial on
 * thread 0 between two barriers: the greedy pair walk and the group
 * boundaries, which read the labels' times from the workspace.
 *
 * Memory: a recording of at most A.lds_n raw peaks keeps its workspace in LDS
 * (bpmx_plan.h: 40 KB, four workgroups per CU).  A longer one works in its
 * slice of the global buffer.  The tables are read where they lie: each entry
 * once, the final beats by binary search.  It reads pk_off, n_final, n_bpm and
 * the beats status itself, so nothing synchronises the host.  Nothing is read
 * or written beyond the table capacity: a recording whose slice reaches past
 * it only reports BPMX_LABELS_OVERFLOW.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_labels_core.h"

namespace bpmx {

namespace {
struct labels_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return LABELS_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(LABELS_T) void k_labels(LabelsArgs A) {
    extern __shared__ __align__(16) unsigned char labels_lds[];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t o = A.pk_off[f], e = A.pk_off[f + 1], n = e - o;
    if (o < 0 || n < 0 || e > A.cap) {
        if (lane == 0) A.O.status[f] = BPMX_LABELS_OVERFLOW;
        return;
    }
    int64_t nf = A.n_final[f], m = A.n_bpm[f];
    /* a beats status other than OK, or counts its slice cannot hold: no labels */
    if (A.b_status[f] != BPMX_HOST_OK || nf < 0 || nf > n || m < 0 || (m > 0 && m >= nf)) nf = m = 0;
    const bool in_lds = n <= A.lds_n;
    void *base = in_lds ? (void *)labels_lds : (void *)(A.gws + (size_t)f * A.fixed + (size_t)o * LB_STRIDE);
    const labels_ws w = labels_ws_layout(base, n, LABELS_T);
    labels_io io;
    io.lb_pos = A.O.lb_pos + o; io.lb_type = A.O.lb_type + o; io.lb_time = A.O.lb_time + o; io.lb_bpm = A.O.lb_bpm + o;
    io.pr_s1 = A.O.pr_s1 + o; io.pr_s2 = A.O.pr_s2 + o; io.pr_dt = A.O.pr_dt + o;
    io.gr_id = A.O.gr_id + o; io.gr_first = A.O.gr_first + o; io.gr_last = A.O.gr_last + o;
    io.gr_s1 = A.O.gr_s1 + o; io.gr_pairs = A.O.gr_pairs + o; io.gr_dt = A.O.gr_dt + o; io.gr_bpm = A.O.gr_bpm + o;
    io.n_labels = A.O.n_labels + f; io.n_pairs = A.O.n_pairs + f; io.n_groups = A.O.n_groups + f;
    io.record = A.O.record + (size_t)f * BPMX_LABELS_RECORD;
    const int rc = labels_core(labels_group(), n, A.pk_idx + o, A.tags + o, A.gap + o, nf, A.final_idx + o, m,
                               A.bpm_t + o, A.bpm + o, A.sr, A.P, w, io);
    if (lane == 0) A.O.status[f] = rc;
}

}  // namespace bpmx
