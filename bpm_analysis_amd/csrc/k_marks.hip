/*
 * k_marks.hip — bpmx_marks_device: a person's corrected marks as a peak
 * table, final beats and BPM curve, in three stream-ordered launches.
 *
 *   k_marks_rows    per recording one workgroup of MARKS_T threads: the kept
 *                   marks and the rows of its rf_off slice into scratch, the
 *                   counts into cnt (marks_rows of bpmx_marks_core.h)
 *   k_marks_scan    one workgroup: the exclusive prefix sums of the row counts
 *                   into pk_off, tile after tile of MARKS_T files with a
 *                   carry, as k_pack_scan does for the run's counts
 *   k_marks_finish  per recording one workgroup: the rows to the pk_off
 *                   slice, tags, gap, NaN env / floor, the S1 rows, the curve
 *                   (marks_finish, which runs beats_series of the beats core),
 *                   status and record
 *
 * The logic is bpmx_marks_core.h, the same text the host tests run; this file
 * gives it the workgroup executor and the memory.  k_marks_rows keeps its
 * lane counts in static LDS and works on the scratch slices where they lie.
 * k_marks_finish: a recording of at most A.lds_n S1 rows keeps its workspace
 * in LDS (bpmx_plan.h: 32 KB, five workgroups per CU), a longer one works in
 * its slice of the global buffer.  Nothing is read or written beyond the
 * capacities: a recording whose mark slice reaches past cap_ref (or whose
 * rf_off descends) counts as zero rows, and it or one whose rows reach past
 * cap_peaks only reports BPMX_MARKS_OVERFLOW.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_marks_core.h"

namespace bpmx {

namespace {
struct marks_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return MARKS_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(MARKS_T) void k_marks_rows(MarksArgs A) {
    __shared__ __align__(8) unsigned char head[marks_ws_head(MARKS_T)];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t ro = A.rf_off[f], re = A.rf_off[f + 1], nr = re - ro;
    int32_t *cnt = A.cnt + f * MC_PER_FILE;
    if (ro < 0 || nr < 0 || re > A.cap_ref) {
        if (lane < MC_PER_FILE) cnt[lane] = lane == MC_BAD ? 1 : 0;
        return;
    }
    marks_rows(marks_group(), nr, A.rf_ms + ro, A.rf_type + ro, A.sr, A.nd ? A.nd[f] : (int64_t)-1,
               marks_head_layout(head, MARKS_T), A.k_idx + ro, A.k_type + ro, A.r_idx + ro, A.r_tag + ro, cnt);
}

__global__ __launch_bounds__(MARKS_T) void k_marks_scan(MarksArgs A) {
    constexpr int NW = MARKS_T / 64;
    __shared__ long long wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t F = A.n_files;
    long long carry = 0;
    for (int64_t base = 0; base < F; base += MARKS_T) {
        const int64_t f = base + tid;
        const long long c = f < F ? (long long)A.cnt[f * MC_PER_FILE + BPMX_MK_N_ROWS] : 0;
        long long v = c;                       /* inclusive scan within the wave */
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(v, d, 64);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long long pre = 0, tot = 0;
        for (int k = 0; k < NW; ++k) {
            const long long x = wsum[k];
            if (k < wave) pre += x;
            tot += x;
        }
        if (f < F) A.pk_off[f] = carry + pre + v - c;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) A.pk_off[F] = carry;
}

__global__ __launch_bounds__(MARKS_T) void k_marks_finish(MarksArgs A) {
    extern __shared__ __align__(16) unsigned char marks_lds[];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t ro = A.rf_off[f], re = A.rf_off[f + 1], nr = re - ro;
    const int32_t *cnt = A.cnt + f * MC_PER_FILE;
    const int64_t o = A.pk_off[f], n = cnt[BPMX_MK_N_ROWS], ns1 = cnt[BPMX_MK_N_S1];
    /* the counts are k_marks_rows' own: never more rows than marks, never more S1 rows than rows */
    if (ro < 0 || nr < 0 || re > A.cap_ref || cnt[MC_BAD] || n < 0 || n > nr || ns1 < 0 || ns1 > n || o < 0 ||
        o + n > A.cap) {
        if (lane == 0) A.B.status[f] = BPMX_MARKS_OVERFLOW;
        return;
    }
    const bool in_lds = ns1 <= A.lds_n;
    unsigned char *base = in_lds ? marks_lds : A.gws + (size_t)f * A.fixed + (size_t)ro * MK_STRIDE;
    const marks_head h = marks_head_layout(base, MARKS_T);
    const beats_ws w = beats_ws_layout(base + marks_ws_head(MARKS_T), ns1, false);
    marks_io io;
    io.pk_idx = A.pk_idx + o;
    io.pk_env = A.pk_env ? A.pk_env + o : nullptr;
    io.pk_floor = A.pk_floor ? A.pk_floor + o : nullptr;
    io.tags = A.B.tags + o; io.gap = A.gap + o;
    io.final_idx = A.B.final_idx + o; io.n_final = A.B.n_final + f;
    io.bpm_t = A.B.bpm_t + o; io.bpm = A.B.bpm + o; io.n_bpm = A.B.n_bpm + f;
    io.pass = A.B.pass ? A.B.pass + 3 * f : nullptr;
    io.record = A.record + f * BPMX_MARKS_RECORD;
    const int rc = marks_finish(marks_group(), n, A.r_idx + ro, A.r_tag + ro, cnt, A.sr, A.window_sec, h, w, io);
    if (lane == 0) A.B.status[f] = rc;
}

}  // namespace bpmx
