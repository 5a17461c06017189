/*
 * k_beats.hip — bpmx_beats_device: the beat stages (preliminary pass,
 * classifier, refinement, BPM curve) on the packed per-peak tables, one wave64
 * workgroup per recording.
 *
 * The logic is bpmx_beats_core.h, the same text the host tests run; this file
 * gives it the wave executor and the memory.  The classifier walk, the Kahan
 * rolling means and the refinement passes depend on their own earlier steps:
 * they run on lane 0 between two barriers.  The gathers (strength, raw
 * deviation, dev_t, RR arrays, window bounds), the bitonic sorts behind every
 * median and percentile, and the copies out use all 64 lanes.
 *
 * Memory: a recording of at most A.lds_n peaks keeps its workspace and a copy
 * of idx and env_pk in LDS (bpmx_plan.h: 40 KB, four workgroups per CU); the
 * floor is read where it lies (twice per peak, and in the rare gap fill).  A
 * longer table works in its slice of the global buffer and reads idx and env_pk
 * from the tables.  Nothing is read or written beyond the table capacity: a
 * recording whose slice reaches past it only reports BPMX_BEATS_OVERFLOW.
 *
 * k_beats_hints and k_beats_trace (bpmx_beats_device_ex) are the same stages
 * with a start hint per recording and, k_beats_trace, the decision trace
 * written to HBM as it is decided; k_beats itself takes neither.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_beats_core.h"

namespace bpmx {

namespace {
struct beats_wave {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return BEATS_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(BEATS_T) void k_beats(BeatsArgs A) {
    extern __shared__ __align__(16) unsigned char beats_lds[];
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t o = A.pk_off[f], e = A.pk_off[f + 1], n = e - o;
    int32_t st = BPMX_HOST_OK;
    if (A.flags && (A.flags[f] & (BPMX_F_TOO_SHORT | BPMX_F_BAD_WINDOW))) st = BPMX_BEATS_SKIPPED;
    else if (o < 0 || n < 0 || e > A.cap) st = BPMX_BEATS_OVERFLOW;
    double *pass = A.pass ? A.pass + 3 * f : nullptr;
    if (st != BPMX_HOST_OK) {
        if (lane == 0) {
            A.n_final[f] = 0;
            A.n_bpm[f] = 0;
            A.status[f] = st;
            if (pass) pass[0] = pass[1] = pass[2] = bc_nan();
        }
        return;
    }
    const bool in_lds = n <= A.lds_n;
    void *base = in_lds ? (void *)beats_lds
                        : (void *)(A.gws + (size_t)f * BEATS_WS_FIXED + (size_t)o * BEATS_WS_STRIDE);
    const beats_ws w = beats_ws_layout(base, n, in_lds);
    const int32_t *idx = A.pk_idx + o;
    const double *env = A.pk_env + o, *flo = A.pk_floor + o;
    if (in_lds) {
        for (int64_t i = lane; i < n; i += BEATS_T) {
            w.idx_stage[i] = idx[i];
            w.env_stage[i] = env[i];
        }
        __syncthreads();
        idx = w.idx_stage;
        env = w.env_stage;
    }
    const int rc = beats_core(beats_wave(), n, idx, env, flo, A.sr, A.P, A.hint, w, A.final_idx + o, A.n_final + f,
                              A.bpm_t + o, A.bpm + o, A.n_bpm + f, pass, A.tags ? A.tags + o : nullptr);
    if (lane == 0) A.status[f] = rc;
}

/* bpmx_beats_device_ex: k_beats' text with a per-file hint and, TRACE, the
 * decision trace as the sink of bpmx_beats_core.h.  Same workspace, same LDS
 * layout and budget: the trace goes to HBM where it is decided (lane 0's plain
 * stores in the serial parts, all lanes for dev_t / dev / gap); nothing loads
 * it back, so the stores are off the dependent chain.  A recording that is
 * skipped or overflows returns before anything of the trace is touched. */
namespace {
template <bool TRACE>
__device__ __forceinline__ void beats_ex_body(const BeatsArgs &A, const BeatsExArgs &E, unsigned char *lds) {
    const int64_t f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t o = A.pk_off[f], e = A.pk_off[f + 1], n = e - o;
    int32_t st = BPMX_HOST_OK;
    if (A.flags && (A.flags[f] & (BPMX_F_TOO_SHORT | BPMX_F_BAD_WINDOW))) st = BPMX_BEATS_SKIPPED;
    else if (o < 0 || n < 0 || e > A.cap) st = BPMX_BEATS_OVERFLOW;
    double *pass = A.pass ? A.pass + 3 * f : nullptr;
    if (st != BPMX_HOST_OK) {
        if (lane == 0) {
            A.n_final[f] = 0;
            A.n_bpm[f] = 0;
            A.status[f] = st;
            if (pass) pass[0] = pass[1] = pass[2] = bc_nan();
        }
        return;
    }
    const bool in_lds = n <= A.lds_n;
    void *base = in_lds ? (void *)lds : (void *)(A.gws + (size_t)f * BEATS_WS_FIXED + (size_t)o * BEATS_WS_STRIDE);
    const beats_ws w = beats_ws_layout(base, n, in_lds);
    const int32_t *idx = A.pk_idx + o;
    const double *env = A.pk_env + o, *flo = A.pk_floor + o;
    if (in_lds) {
        for (int64_t i = lane; i < n; i += BEATS_T) {
            w.idx_stage[i] = idx[i];
            w.env_stage[i] = env[i];
        }
        __syncthreads();
        idx = w.idx_stage;
        env = w.env_stage;
    }
    const double hint = E.hints ? E.hints[f] : A.hint;
    int rc;
    if (TRACE) {
        beats_trace tr;
        tr.rec = E.record + o * BPMX_TR_NFIELDS;
        tr.code = E.code + o; tr.lt_pos = E.lt_pos + o; tr.lt_bpm = E.lt_bpm + o; tr.n_lt = E.n_lt + f;
        tr.dev_t = E.dev_t + o; tr.dev = E.dev + o; tr.gap = E.gap + o;
        rc = beats_core(beats_wave(), n, idx, env, flo, A.sr, A.P, hint, w, A.final_idx + o, A.n_final + f,
                        A.bpm_t + o, A.bpm + o, A.n_bpm + f, pass, A.tags ? A.tags + o : nullptr, tr);
    } else {
        rc = beats_core(beats_wave(), n, idx, env, flo, A.sr, A.P, hint, w, A.final_idx + o, A.n_final + f,
                        A.bpm_t + o, A.bpm + o, A.n_bpm + f, pass, A.tags ? A.tags + o : nullptr);
    }
    if (lane == 0) A.status[f] = rc;
}
}  // namespace

__global__ __launch_bounds__(BEATS_T) void k_beats_hints(BeatsArgs A, BeatsExArgs E) {
    extern __shared__ __align__(16) unsigned char beats_lds[];
    beats_ex_body<false>(A, E, beats_lds);
}

__global__ __launch_bounds__(BEATS_T) void k_beats_trace(BeatsArgs A, BeatsExArgs E) {
    extern __shared__ __align__(16) unsigned char beats_lds[];
    beats_ex_body<true>(A, E, beats_lds);
}

}  // namespace bpmx
