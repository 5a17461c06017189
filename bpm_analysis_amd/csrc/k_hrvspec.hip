/*
 * k_hrvspec.hip — bpmx_hrvspec_device: the HRV spectrum of a ragged batch in
 * two stream-ordered launches.
 *
 *   k_hrvspec<B, PARTS, ROT>  one workgroup of HRVSPEC_T threads per
 *                    (recording, window) pair, found by bisection over the
 *                    window offsets.  The workgroup bisects the recording's
 *                    final beats for its span and stages s_j, u_j and, with
 *                    ROT, (cos, sin)(dom * s_j) of the kept intervals in LDS
 *                    (hrvspec_stage).  Lanes own frequencies: PARTS adjacent
 *                    lanes share a block of B consecutive frequencies and
 *                    split the intervals among them, so the workgroup covers
 *                    HRVSPEC_T / PARTS * B frequencies a pass and any n_freq
 *                    in as many passes as it takes.  ROT: one sincos per
 *                    interval and block, then B - 1 rotations by dom * s_j
 *                    along the grid; else one sincos per term.  The six sums
 *                    of the PARTS lanes meet by shuffles in a fixed order that
 *                    leaves each lane one frequency to finish, q goes to LDS
 *                    (and to out.q), and the band sums and peaks are trees
 *                    over the workgroup (hrvspec_band).
 *   k_hrvspec_record one wave per recording: the status and the record, read
 *                    from the per-window arrays where they lie, 64 windows at
 *                    a time, so any window count works.
 *
 * The kernels read pk_off, n_final and the beats status themselves, so nothing
 * synchronises the host.  Nothing outside [0, window total) of the per-window
 * arrays is written; final_idx is read only inside the file's slice, which is
 * checked against cap first: a recording whose slice reaches past it only
 * reports BPMX_HRVSPEC_OVERFLOW.  LDS: at most nmax intervals are staged
 * (hrvspec_stage clamps), nmax * HRVSPEC_PER bytes were checked by the host.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_hrvspec_core.h"

namespace bpmx {

namespace {
struct hrvspec_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return HRVSPEC_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    /* flag is 0 or 1; ws: HRVSPEC_T / 64 entries at least */
    __device__ __forceinline__ int count(int flag, int32_t *ws, int *total) const {
        const unsigned long long m = __ballot(flag != 0);
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) ws[wave] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (int k = 0; k < HRVSPEC_T / 64; ++k) {
            const int c = ws[k];
            before += k < wave ? c : 0;
            all += c;
        }
        *total = all;
        return before;
    }
};
struct hrvspec_wave {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return HRVSPEC_REC_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

/* 0: a slice to work on, 1: no beats to use, 2: the slice reaches past cap */
__device__ __forceinline__ int file_state(const HrvspecArgs &A, int64_t f, int64_t *o, int64_t *nf) {
    const int64_t a = A.pk_off[f], e = A.pk_off[f + 1], n = e - a;
    if (a < 0 || n < 0 || e > A.cap) return 2;
    const int64_t k = A.n_final[f];
    *o = a;
    *nf = k;
    if (A.b_status[f] != BPMX_HOST_OK || k < 2 || k > n) return 1;
    return 0;
}
}  // namespace

template <int B, int PARTS, bool ROT>
__global__ __launch_bounds__(HRVSPEC_T) void k_hrvspec(HrvspecArgs A) {
    extern __shared__ __align__(16) double hrvspec_lds[];
    __shared__ double s_q[HRVSPEC_MAX_FREQ];
    __shared__ double s_dw[HRVSPEC_T];
    __shared__ int32_t s_iw[HRVSPEC_T];
    __shared__ hrvspec_pick s_pk[HRVSPEC_T];
    static_assert(PARTS == B && PARTS <= 64 && (PARTS & (PARTS - 1)) == 0, "as many lanes as frequencies per block, in one wave");
    const int tid = (int)threadIdx.x;
    const bpmx_hrvspec_params &P = A.P;
    const int nq = P.n_freq;

    /* the recording of this window: woff[f] <= b < woff[f + 1] */
    const int64_t b = blockIdx.x;
    int lo = 0, hi = A.n_files;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.woff[mid] <= b) lo = mid; else hi = mid;
    }
    const int64_t f = lo, wdw = b - A.woff[lo];
    int64_t o = 0, nf = 0;
    const int state = file_state(A, f, &o, &nf);
    if (state == 2) return;                     /* the same decision in every thread */
    if (state == 1) nf = 0;

    hrvspec_ws w;
    hrvspec_ws_intervals(w, hrvspec_lds, A.G.nmax);
    w.dw = s_dw; w.iw = s_iw; w.pk = s_pk;
    const hrvspec_group X;
    const hrvspec_head H = hrvspec_stage(X, A.final_idx + o, nf, wdw * (int64_t)P.hop, P, A.sr, A.G.nmax, ROT, w);
    double *qrow = A.O.q ? A.O.q + b * (int64_t)nq : nullptr;
    if (H.code != 0) {
        if (tid == 0) {
            A.O.code[b] = H.code; A.O.n_rr[b] = H.n; A.O.lf_peak[b] = -1; A.O.hf_peak[b] = -1;
            A.O.t_mid[b] = H.t_mid; A.O.var[b] = hs_nan(); A.O.lf[b] = hs_nan(); A.O.hf[b] = hs_nan();
        }
        if (qrow)
            for (int m = tid; m < nq; m += HRVSPEC_T) qrow[m] = hs_nan();
        return;
    }

    /* the six sums: PARTS adjacent lanes per block of B frequencies */
    constexpr int PER_PASS = HRVSPEC_T / PARTS * B;
    const int g = tid / PARTS, p = tid % PARTS;
    for (int base = 0; base < nq; base += PER_PASS) {
        const int m0 = base + g * B;
        double acc[HS_NSUM][B];
#pragma unroll
        for (int i = 0; i < HS_NSUM; ++i)
#pragma unroll
            for (int k = 0; k < B; ++k) acc[i][k] = 0.0;
        if (m0 < nq) hrvspec_accum<B, ROT>(w, H.n, p, PARTS, m0, P, acc);
        /* reduce and scatter: after the step of h lanes, a lane keeps the h frequencies of its half; at the
           end lane p of the block holds the sums of frequency p of it */
#pragma unroll
        for (int h = B / 2; h >= 1; h >>= 1) {
            const bool up = (p & h) != 0;
#pragma unroll
            for (int i = 0; i < HS_NSUM; ++i)
#pragma unroll
                for (int k = 0; k < h; ++k) {
                    const double mine = up ? acc[i][k + h] : acc[i][k], send = up ? acc[i][k] : acc[i][k + h];
                    acc[i][k] = mine + __shfl_xor(send, h, 64);
                }
        }
        if (m0 + p < nq) {
            double sum[HS_NSUM];
#pragma unroll
            for (int i = 0; i < HS_NSUM; ++i) sum[i] = acc[i][0];
            const double q = hrvspec_power(sum, H.n, H.Y, H.YY);
            s_q[m0 + p] = q;
            if (qrow) qrow[m0 + p] = q;
        }
    }
    __syncthreads();

    const hrvspec_bandval lf = hrvspec_band(X, s_q, P.lf_a, P.lf_b, w);
    const hrvspec_bandval hf = hrvspec_band(X, s_q, P.hf_a, P.hf_b, w);
    if (tid == 0) {
        const double k = P.scale * (H.e_last - H.e_first) * H.var;
        A.O.code[b] = 0; A.O.n_rr[b] = H.n; A.O.lf_peak[b] = lf.peak; A.O.hf_peak[b] = hf.peak;
        A.O.t_mid[b] = H.t_mid; A.O.var[b] = H.var;
        A.O.lf[b] = P.lf_b > P.lf_a ? k * lf.sum : 0.0;
        A.O.hf[b] = P.hf_b > P.hf_a ? k * hf.sum : 0.0;
    }
}

template __global__ void k_hrvspec<HRVSPEC_B, HRVSPEC_PARTS, true>(HrvspecArgs A);
template __global__ void k_hrvspec<1, 1, false>(HrvspecArgs A);

__global__ __launch_bounds__(HRVSPEC_REC_T) void k_hrvspec_record(HrvspecArgs A) {
    __shared__ double st[3 * HRVSPEC_REC_T];
    const int64_t f = blockIdx.x;
    int64_t o = 0, nf = 0;
    const int state = file_state(A, f, &o, &nf);
    if (state == 2) {
        if (threadIdx.x == 0) A.O.status[f] = BPMX_HRVSPEC_OVERFLOW;
        return;
    }
    const int64_t w0 = A.woff[f], nw = A.woff[f + 1] - w0;
    hrvspec_record(hrvspec_wave(), nw, A.O.code + w0, A.O.lf + w0, A.O.hf + w0, st,
                   A.O.record + f * (int64_t)BPMX_HRVSPEC_RECORD);
    if (threadIdx.x == 0) A.O.status[f] = state == 1 ? BPMX_HRVSPEC_NONE : BPMX_HRVSPEC_OK;
}

}  // namespace bpmx
