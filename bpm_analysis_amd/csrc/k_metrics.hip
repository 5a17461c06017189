/*
 * k_metrics.hip — bpmx_metrics_device: the final metrics (windowed HRV table,
 * summary, heart-rate recovery, steepest recovery and exertion slopes, major
 * inclines and declines) from k_beats' outputs where they lie, one workgroup
 * of METRICS_T threads per recording.
 *
 * The logic is bpmx_metrics_core.h, the same text the host tests run; this
 * file gives it the workgroup executor and the memory.  Parallel: the index
 * times, one HRV window per thread, the curve's extremes, one start of the
 * steepest-slope search per thread, the extrema scan, the ranks behind the
 * distance filter's visiting order, the prominence walks, the tie test, the
 * run pairing and the runs' rank sort.  Serial on thread 0 between two
 * barriers: the pairwise sums of the summary, the HRR interpolation, the
 * compactions and the greedy distance filter.
 *
 * Memory: a recording of at most A.lds_n raw peaks keeps its workspace and a
 * copy of its curve and beats in LDS (bpmx_plan.h: 48 KB, three workgroups per
 * CU).  A longer one works in its slice of the global buffer and reads the
 * curve and the beats where k_beats left them.  It reads pk_off, n_final,
 * n_bpm and the beats status itself, so nothing synchronises the host.
 * Nothing is read or written beyond the table capacity: a recording whose
 * slice reaches past it only reports BPMX_METRICS_OVERFLOW.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_metrics_core.h"

namespace bpmx {

namespace {
struct metrics_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return METRICS_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(METRICS_T) void k_metrics(MetricsArgs A) {
    extern __shared__ __align__(16) unsigned char metrics_lds[];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t o = A.pk_off[f], e = A.pk_off[f + 1], n = e - o;
    if (o < 0 || n < 0 || e > A.cap) {
        if (lane == 0) A.O.status[f] = BPMX_METRICS_OVERFLOW;
        return;
    }
    int64_t nf = A.n_final[f], m = A.n_bpm[f];
    /* a beats status other than OK, or counts its slice cannot hold: no metrics */
    if (A.b_status[f] != BPMX_HOST_OK || nf < 0 || nf > n || m < 0 || (m > 0 && m >= nf)) nf = m = 0;
    const bool in_lds = n <= A.lds_n;
    void *base = in_lds ? (void *)metrics_lds : (void *)(A.gws + (size_t)f * A.fixed + (size_t)o * MX_STRIDE);
    const metrics_ws w = metrics_ws_layout(base, n, METRICS_T, A.fw, in_lds);
    const int32_t *fin = A.final_idx + o;
    const double *bt = A.bpm_t + o, *v = A.bpm + o;
    if (in_lds) {
        for (int64_t i = lane; i < nf; i += METRICS_T) w.fin_stage[i] = fin[i];
        for (int64_t i = lane; i < m; i += METRICS_T) w.v_stage[i] = v[i];
        __syncthreads();
        fin = w.fin_stage;
        v = w.v_stage;
    }
    metrics_io io;
    io.hrv_time = A.O.hrv_time + o; io.hrv_rmssdc = A.O.hrv_rmssdc + o;
    io.hrv_sdnn = A.O.hrv_sdnn + o; io.hrv_bpm = A.O.hrv_bpm + o;
    io.n_hrv = A.O.n_hrv + f;
    io.inc_a = A.O.inc_a + o; io.inc_b = A.O.inc_b + o; io.dec_a = A.O.dec_a + o; io.dec_b = A.O.dec_b + o;
    io.inc_slope = A.O.inc_slope + o; io.inc_dur = A.O.inc_dur + o;
    io.dec_slope = A.O.dec_slope + o; io.dec_dur = A.O.dec_dur + o;
    io.n_inc = A.O.n_inc + f; io.n_dec = A.O.n_dec + f;
    io.record = A.O.record + (size_t)f * BPMX_METRICS_RECORD;
    const int rc = metrics_core(metrics_group(), nf, fin, m, bt, v, A.sr, A.P, A.epoch_us, w, io);
    if (lane == 0) A.O.status[f] = rc;
}

}  // namespace bpmx
