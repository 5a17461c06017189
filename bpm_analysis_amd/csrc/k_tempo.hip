/*
 * k_tempo.hip — bpmx_tempo_device: the tempogram of a ragged batch in two
 * stream-ordered launches.
 *
 *   k_tempo_valu<L>  one workgroup of TEMPO_T threads per (recording, window)
 *                    pair.  The window is read once from HBM, checked
 *                    (tempo_scan), mean-removed and kept zero-padded in LDS;
 *                    the lag sums r[kmin - 1 .. kmax + 1] come from there.  A
 *                    lane holds L consecutive lags in registers: a step of
 *                    TEMPO_U window samples costs TEMPO_U broadcast reads and
 *                    TEMPO_U new reads of the sliding e[i + k ..] window for
 *                    TEMPO_U * L fused multiply-adds.  L is odd, so the lanes'
 *                    8-byte reads at a stride of L doubles fall on distinct
 *                    banks.  The four waves each take a quarter of the window
 *                    and leave partial sums in LDS, added in wave order.  The
 *                    pick and the outputs are bpmx_tempo_core.h.
 *   k_tempo_record   one wave per recording: counts, median by rank counting,
 *                    mean, hint (tempo_record), read from the per-window
 *                    arrays where they lie, so any window count works.
 *
 * Nothing outside [0, window total) of the per-window arrays is written, and
 * nothing is read outside a window's win samples of its recording's slice:
 * the last window ends at or before nd by bpmx_tempo_windows.  LDS reads stay
 * below elen = win4 + kmax + TEMPO_PAD: a lane's last lag is at most
 * kmax + 1 + (L - 1), its last window sample win4 - 1.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_tempo_core.h"

namespace bpmx {

namespace {
struct tempo_group {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return TEMPO_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
struct tempo_wave {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return TEMPO_REC_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

/* the sum of v over the workgroup, the same value in every thread; slot: TEMPO_WAVES doubles */
__device__ __forceinline__ double group_sum(double v, double *slot) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int k = 1; k < TEMPO_WAVES; ++k) s += slot[k];
    return s;
}
}  // namespace

template <int L>
__global__ __launch_bounds__(TEMPO_T) void k_tempo_valu(TempoArgs A) {
    extern __shared__ __align__(16) double tempo_lds[];
    __shared__ double s_sum[TEMPO_WAVES];
    __shared__ tempo_scan s_scan[TEMPO_WAVES];
    __shared__ tempo_best s_best[TEMPO_T];
    constexpr int U = TEMPO_U;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int win = A.P.win, kmin = A.P.kmin, kmax = A.P.kmax;
    const int nlag = A.G.nlag, elen = A.G.elen, pstride = A.G.pstride;
    double *e = tempo_lds, *part = tempo_lds + elen;

    /* the recording of this window: woff[f] <= b < woff[f + 1] */
    const int64_t b = blockIdx.x;
    int lo = 0, hi = A.n_files;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.woff[mid] <= b) lo = mid; else hi = mid;
    }
    const double *x = A.env + A.doff[lo] + (b - A.woff[lo]) * (int64_t)A.P.hop;

    /* step 1 and the window into LDS */
    tempo_scan sc = tempo_scan_init();
    double sum = 0.0;
    for (int i = tid; i < win; i += TEMPO_T) {
        const double v = x[i];
        e[i] = v;
        tempo_scan_add(sc, v);
        sum += v;
    }
    for (int i = win + tid; i < elen; i += TEMPO_T) e[i] = 0.0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        tempo_scan o;
        o.mn = __shfl_xor(sc.mn, d, 64);
        o.mx = __shfl_xor(sc.mx, d, 64);
        o.bad = __shfl_xor(sc.bad, d, 64);
        tempo_scan_merge(sc, o);
    }
    if (lane == 0) s_scan[wave] = sc;
    __syncthreads();
    sc = s_scan[0];
#pragma unroll
    for (int k = 1; k < TEMPO_WAVES; ++k) tempo_scan_merge(sc, s_scan[k]);
    if (!tempo_scan_valid(sc)) {            /* the same decision in every thread */
        if (tid == 0) {
            const tempo_val v = tempo_outputs(0, 0.0, 0.0, 0.0, 0.0, A.sr);
            A.O.lag[b] = v.lag; A.O.rho[b] = v.rho; A.O.bpm[b] = v.bpm;
        }
        return;
    }

    /* step 2: the mean of finite samples; r[0] */
    const double m = group_sum(sum, s_sum) / (double)win;
    double sq = 0.0;
    for (int i = tid; i < win; i += TEMPO_T) {
        const double v = e[i] - m;
        e[i] = v;
        sq = __builtin_fma(v, v, sq);
    }
    const double r0 = group_sum(sq, s_sum);     /* its barriers order the writes of e before the reads below */

    /* step 3: wave w over the window samples [w * chunk, (w + 1) * chunk) below win4 */
    const int i0 = wave * A.G.chunk;
    const int i1 = i0 + A.G.chunk < A.G.win4 ? i0 + A.G.chunk : A.G.win4;
    double *mine = part + (size_t)wave * pstride;
    for (int base = 0; base < nlag; base += 64 * L) {
        const int j0 = base + lane * L;
        if (j0 >= nlag) continue;
        const double *p = e + (kmin - 1 + j0);
        double acc[L], wv[L + U - 1];
#pragma unroll
        for (int l = 0; l < L; ++l) acc[l] = 0.0;
        if (i0 < i1) {
#pragma unroll
            for (int t = 0; t < L - 1; ++t) wv[t] = p[i0 + t];
        }
        for (int i = i0; i < i1; i += U) {
            double a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = e[i + u];
#pragma unroll
            for (int u = 0; u < U; ++u) wv[L - 1 + u] = p[i + L - 1 + u];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int l = 0; l < L; ++l) acc[l] = __builtin_fma(a[u], wv[u + l], acc[l]);
#pragma unroll
            for (int t = 0; t < L - 1; ++t) wv[t] = wv[t + U];
        }
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (j0 + l < nlag) mine[j0 + l] = acc[l];
    }
    __syncthreads();
    for (int j = tid; j < nlag; j += TEMPO_T) {
        double s = part[j];
#pragma unroll
        for (int k = 1; k < TEMPO_WAVES; ++k) s += part[(size_t)k * pstride + j];
        part[j] = s;
    }
    __syncthreads();

    /* steps 4 to 6 */
    const tempo_best best = tempo_pick(tempo_group(), part, kmin, kmax, s_best);
    if (tid == 0) {
        tempo_val v;
        if (best.k == 0) {
            v = tempo_outputs(0, 0.0, 0.0, 0.0, 0.0, A.sr);
        } else {
            const int j = best.k - (kmin - 1);
            v = tempo_outputs(best.k, part[j - 1], part[j], part[j + 1], r0, A.sr);
        }
        A.O.lag[b] = v.lag; A.O.rho[b] = v.rho; A.O.bpm[b] = v.bpm;
    }
}

template __global__ void k_tempo_valu<5>(TempoArgs A);
template __global__ void k_tempo_valu<7>(TempoArgs A);

__global__ __launch_bounds__(TEMPO_REC_T) void k_tempo_record(TempoArgs A) {
    __shared__ __align__(8) unsigned char ws[tempo_rec_ws_bytes(TEMPO_REC_T)];
    const int64_t f = blockIdx.x;
    const int64_t o = A.woff[f], nw = A.woff[f + 1] - o;
    tempo_rec r;
    r.n_valid = A.O.n_valid + f; r.n_strong = A.O.n_strong + f;
    r.median_bpm = A.O.median_bpm + f; r.mean_rho = A.O.mean_rho + f; r.hint = A.O.hint + f;
    tempo_record(tempo_wave(), nw, A.O.lag + o, A.O.rho + o, A.O.bpm + o, A.P.min_strength, A.P.start_windows,
                 tempo_rec_ws_layout(ws, TEMPO_REC_T), r);
}

}  // namespace bpmx
