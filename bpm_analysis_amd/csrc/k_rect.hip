/*
 * k_rect.hip — rectified-mode envelope: the labeler's envelope of a filtered
 * WAV (heartbeat_labeler.py:53-67), bit-exact:
 *   a = np.abs(frame value) in its dtype, no decimation, no filter,
 *   env = pd.Series(a).rolling(w, min_periods=1, center=True).mean().
 *
 * Exact-integer route (u8 / i16 / i32, one or two channels; the argument is in
 * bpmx_plan.h at rect_plan): env[i] = (P[e] - P[s]) [* 0.5] / (e - s) with P the
 * integer prefix sums of the rectified frames.  Memory-bound: 16-byte PCM loads
 * where a vector holds whole frames, contiguous f64 stores, the prefix in LDS.
 *   k_rect_lds   one workgroup per (recording, chunk of RECT_CHUNK outputs):
 *                the chunk's inputs with their halo (chunk + w - 1 frames)
 *                into LDS, a block scan, the outputs.
 *   k_rect_csum / k_rect_cscan / k_rect_gout   windows beyond the LDS: sums of
 *                chunks of inputs, their exclusive scan per recording, and a
 *                pass that rebuilds the prefix over the (at most two) chunks
 *                around its window starts, then around its window ends, each
 *                from the scanned chunk sum.  Stream-ordered launches carry the
 *                sums between workgroups; none waits on another.
 * General route (any dtype and channel count): k_rect_pick gathers the
 * rectified values (inf -> NaN) into rows [frame][recording], k_rect_seq runs
 * the pandas recursion (bpmx_rect_core.h rect_roll_mean over RollMean) with
 * one lane per recording.  It only has to be right.
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_rect_core.h"

namespace bpmx {

namespace {

/* T: the sample type; A: the type of a workgroup's local prefix sums in LDS.
 * A workgroup sums at most RECT_LDS_N rectified frames, each at most 2^16 for
 * u8 / i16 (|l + r| of two int16), so 32 bits hold them (RECT_LDS_N * 2^16 <
 * 2^31): half the LDS bytes and traffic, twice the workgroups per CU.  int32
 * PCM needs 64 bits.  Sums across chunks (k_rect_csum) are always int64. */
template <int DT> struct RPcm;
template <> struct RPcm<BPMX_DT_U8> { typedef uint8_t T; typedef int32_t A; };
template <> struct RPcm<BPMX_DT_I16> { typedef int16_t T; typedef int32_t A; };
template <> struct RPcm<BPMX_DT_I32> { typedef int32_t T; typedef int64_t A; };
template <> struct RPcm<BPMX_DT_I24> { typedef pcm24 T; typedef int64_t A; };   /* the int32 samples v << 8 (bpmx_pcm.h) */
static_assert(RECT_LDS_N * 65536 < (int64_t(1) << 31), "32-bit local prefixes");

/* the rectified integers of the m frames from absolute frame fr0 into sh[0, m).
 * Where the first frame's address is a multiple of the frame size, a 16-byte
 * vector holds whole frames: the frames up to the next 16-byte boundary and
 * those after the last whole vector are loaded one by one, so nothing outside
 * [fr0, fr0 + m) is read. */
template <int DT, bool ST>
__device__ __forceinline__ void rect_load(const void *__restrict__ pcm, int64_t fr0, int m,
                                          typename RPcm<DT>::A *sh) {
    typedef typename RPcm<DT>::T T;
    typedef typename RPcm<DT>::A A;
    constexpr int C = ST ? 2 : 1;
    constexpr int FB = (int)sizeof(T) * C;           /* bytes per frame: 1, 2, 4 or 8; packed 24-bit: 3 or 6 */
    constexpr int FPV = 16 / FB;
    constexpr int WDT = DT == BPMX_DT_I24 ? BPMX_DT_I32 : DT;    /* np.abs wraps in the working dtype */
    const char *p = (const char *)pcm + fr0 * FB;
    const uintptr_t a = (uintptr_t)p;
    int head = m, nvec = 0;
    if (16 % FB == 0 && a % FB == 0) {               /* packed 24-bit frames straddle the vectors: one by one */
        head = (int)(((16 - (a & 15)) & 15) / FB);
        if (head > m) head = m;
        nvec = (m - head) / FPV;
    }
    const int tail = head + nvec * FPV;
    const int tid = threadIdx.x;
    auto one = [&](int j) { sh[j] = (A)rect_int_frame<T>(WDT, ST, (const T *)(p + (int64_t)j * FB)); };
    for (int j = tid; j < head; j += RECT_T) one(j);
    const uint4 *__restrict__ pv = (const uint4 *)(p + (int64_t)head * FB);
    for (int v = tid; v < nvec; v += RECT_T) {
        const uint4 q = pv[v];
        T e[(16 + sizeof(T) - 1) / sizeof(T)];       /* nvec is 0 for packed 24-bit */
        __builtin_memcpy(e, &q, 16);
#pragma unroll
        for (int k = 0; k < FPV; ++k) sh[head + v * FPV + k] = (A)rect_int_frame<T>(WDT, ST, e + k * C);
    }
    for (int j = tail + tid; j < m; j += RECT_T) one(j);
}

__device__ __forceinline__ int64_t wave_iscan(int64_t v) {
    const int lane = lane_id();
    long long x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}
__device__ __forceinline__ int32_t wave_iscan(int32_t v) { return wave_iscan_dpp<false>(v); }

/* sh[0, m) hold values on entry (all written, barrier passed); on exit
 * sh[j] = sum of the values below j for j in [0, m].  Each thread owns K
 * consecutive entries; K is odd so that the threads' accesses at stride K fall
 * into different LDS banks.  wtot: RECT_T / 64 entries.  Every thread of the
 * workgroup calls it (the 32-bit wave scan needs whole waves).  Ends with a
 * barrier. */
template <typename A>
__device__ __forceinline__ void rect_scan(A *sh, int m, A *wtot) {
    const int tid = threadIdx.x, wv = tid >> 6;
    const int K = ((m + RECT_T) / RECT_T) | 1;       /* >= ceil((m + 1) / RECT_T) */
    const int j0 = tid * K;
    const int j1 = j0 + K < m ? j0 + K : m;
    A loc = 0;
    for (int j = j0; j < j1; ++j) loc += sh[j];
    const A x = wave_iscan(loc);
    if ((tid & 63) == 63) wtot[wv] = x;
    __syncthreads();
    A p = x - loc;
    for (int k = 0; k < wv; ++k) p += wtot[k];
    const int j2 = j0 + K < m + 1 ? j0 + K : m + 1;
    for (int j = j0; j < j2; ++j) {
        const A v = j < m ? sh[j] : 0;
        sh[j] = p;
        p += v;
    }
    __syncthreads();
}

}  // namespace

template <int DT, bool ST>
__global__ __launch_bounds__(RECT_T) void k_rect_lds(RectArgs G) {
    typedef typename RPcm<DT>::A A;
    extern __shared__ __attribute__((aligned(16))) unsigned char rect_raw[];
    A *rect_sh = (A *)rect_raw;                      /* min(RECT_CHUNK + w, maxn + 1) entries */
    __shared__ A wtot[RECT_T / 64];
    const int f = blockIdx.y;
    const int64_t n = G.doff[f + 1] - G.doff[f], i0 = (int64_t)blockIdx.x * RECT_CHUNK;
    if (!G.active[f] || i0 >= n) return;
    const int64_t i1 = i0 + RECT_CHUNK < n ? i0 + RECT_CHUNK : n, w = G.window;
    int64_t lo, hi, t;
    win_bounds(i0, n, w, lo, t);
    win_bounds(i1 - 1, n, w, t, hi);
    const int m = (int)(hi - lo);                    /* <= i1 - i0 + w - 1 and <= n */
    rect_load<DT, ST>(G.pcm, G.foff[f] + lo, m, rect_sh);
    __syncthreads();
    rect_scan(rect_sh, m, wtot);
    double *__restrict__ env = G.env + G.doff[f];
    for (int64_t i = i0 + threadIdx.x; i < i1; i += RECT_T) {
        int64_t s, e;
        win_bounds(i, n, w, s, e);
        env[i] = rect_mean_exact((int64_t)(rect_sh[e - lo] - rect_sh[s - lo]), e - s, ST);
    }
}

template <int DT, bool ST>
__global__ __launch_bounds__(RECT_T) void k_rect_csum(RectArgs G) {
    typedef typename RPcm<DT>::A A;
    __shared__ A sh[RECT_CHUNK];
    __shared__ int64_t wtot[RECT_T / 64];
    const int f = blockIdx.y;
    const int64_t n = G.doff[f + 1] - G.doff[f], i0 = (int64_t)blockIdx.x * RECT_CHUNK;
    if (!G.active[f] || i0 >= n) return;
    const int m = (int)(n - i0 < RECT_CHUNK ? n - i0 : RECT_CHUNK);
    rect_load<DT, ST>(G.pcm, G.foff[f] + i0, m, sh);
    __syncthreads();
    long long loc = 0;
    for (int j = threadIdx.x; j < m; j += RECT_T) loc += sh[j];
    for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
    if (lane_id() == 0) wtot[wave_id()] = loc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int k = 0; k < RECT_T / 64; ++k) s += wtot[k];
        G.csum[(int64_t)f * G.nch + blockIdx.x] = s;
    }
}

/* one workgroup per recording: its chunk sums -> the sums of all chunks below */
__global__ __launch_bounds__(RECT_T) void k_rect_cscan(RectArgs A) {
    __shared__ int64_t wtot[RECT_T / 64];
    const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6;
    const int64_t n = A.doff[f + 1] - A.doff[f];
    if (!A.active[f] || n < 1) return;
    const int64_t nc = (n + RECT_CHUNK - 1) / RECT_CHUNK;     /* <= A.nch */
    int64_t *cs = A.csum + (int64_t)f * A.nch;
    int64_t carry = 0;
    for (int64_t b = 0; b < nc; b += RECT_T) {
        const int64_t j = b + tid;
        const int64_t v = j < nc ? cs[j] : 0;
        const int64_t x = wave_iscan(v);
        if ((tid & 63) == 63) wtot[wv] = x;
        __syncthreads();
        int64_t ex = carry + x - v, tot = 0;
        for (int k = 0; k < RECT_T / 64; ++k) {
            if (k < wv) ex += wtot[k];
            tot += wtot[k];
        }
        if (j < nc) cs[j] = ex;
        carry += tot;
        __syncthreads();
    }
}

template <int DT, bool ST>
__global__ __launch_bounds__(RECT_T) void k_rect_gout(RectArgs G) {
    typedef typename RPcm<DT>::A A;
    extern __shared__ __attribute__((aligned(16))) unsigned char rect_raw[];
    A *rect_sh = (A *)rect_raw;                      /* 2 RECT_CHUNK entries */
    __shared__ A wtot[RECT_T / 64];
    const int f = blockIdx.y;
    const int64_t n = G.doff[f + 1] - G.doff[f], i0 = (int64_t)blockIdx.x * RECT_CHUNK;
    if (!G.active[f] || i0 >= n) return;
    const int64_t i1 = i0 + RECT_CHUNK < n ? i0 + RECT_CHUNK : n, w = G.window;
    const int64_t nc = (n + RECT_CHUNK - 1) / RECT_CHUNK;
    const int64_t *__restrict__ cs = G.csum + (int64_t)f * G.nch;
    int64_t sa, ea, sb, eb;
    win_bounds(i0, n, w, sa, ea);
    win_bounds(i1 - 1, n, w, sb, eb);
    constexpr int R = (int)(RECT_CHUNK / RECT_T);
    int64_t ps[R];
    /* the local prefix over [A0, last] in LDS: A0 the start of the chunk c that
     * holds `first` (the last chunk when first == n lies past it), so
     * last - A0 <= 2 RECT_CHUNK - 2; P[x] = cs[c] + rect_sh[x - A0] */
    int64_t A0, base;
    auto prefix = [&](int64_t first, int64_t last) {
        int64_t c = first / RECT_CHUNK;
        if (c > nc - 1) c = nc - 1;
        A0 = c * RECT_CHUNK;
        base = cs[c];
        const int m = (int)(last - A0);
        rect_load<DT, ST>(G.pcm, G.foff[f] + A0, m, rect_sh);
        __syncthreads();
        rect_scan(rect_sh, m, wtot);
    };
    prefix(sa, sb);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + threadIdx.x + (int64_t)r * RECT_T;
        int64_t s = sa, e;
        if (i < i1) win_bounds(i, n, w, s, e);
        ps[r] = base + (int64_t)rect_sh[s - A0];
    }
    __syncthreads();
    prefix(ea, eb);
    double *__restrict__ env = G.env + G.doff[f];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + threadIdx.x + (int64_t)r * RECT_T;
        if (i < i1) {
            int64_t s, e;
            win_bounds(i, n, w, s, e);
            env[i] = rect_mean_exact(base + (int64_t)rect_sh[e - A0] - ps[r], e - s, ST);
        }
    }
}

/* rows[r][f] = a_f[r] (inf -> NaN) for a tile of 64 frames x 64 recordings:
 * a wave reads 64 consecutive frames of one recording, the tile goes through
 * LDS, and a wave writes 64 recordings' values of one frame (512 B) */
__global__ __launch_bounds__(256) void k_rect_pick(RectArgs A) {
    __shared__ double tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 64, f0 = (int64_t)blockIdx.y * 64, S = A.n_files;
    for (int fi = wv; fi < 64; fi += 4) {
        const int64_t f = f0 + fi, r = r0 + lane;
        double v = 0.0;
        if (f < S && A.active[f] && r < A.doff[f + 1] - A.doff[f])
            v = rect_value(A.pcm, A.dtype, A.channels, A.foff[f] + r);
        tile[lane][fi] = v;
    }
    __syncthreads();
    for (int ri = wv; ri < 64; ri += 4) {
        const int64_t f = f0 + lane;
        if (f < S) A.rows[(r0 + ri) * S + f] = tile[ri][lane];
    }
}

__global__ __launch_bounds__(64) void k_rect_seq(RectArgs A) {
    const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x, S = A.n_files;
    if (f >= S || !A.active[f]) return;
    const int64_t n = A.doff[f + 1] - A.doff[f];
    const double *__restrict__ v = A.rows + f;
    double *__restrict__ env = A.env + A.doff[f];
    rect_roll_mean(n, (int64_t)A.window, [&](int64_t j) { return v[j * S]; },
                   [&](int64_t i, double m) { env[i] = m; });
}

template __global__ void k_rect_lds<BPMX_DT_U8, false>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_U8, true>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I16, false>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I16, true>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I32, false>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I32, true>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I24, false>(RectArgs);
template __global__ void k_rect_lds<BPMX_DT_I24, true>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_U8, false>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_U8, true>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I16, false>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I16, true>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I32, false>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I32, true>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I24, false>(RectArgs);
template __global__ void k_rect_csum<BPMX_DT_I24, true>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_U8, false>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_U8, true>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I16, false>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I16, true>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I32, false>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I32, true>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I24, false>(RectArgs);
template __global__ void k_rect_gout<BPMX_DT_I24, true>(RectArgs);

}  // namespace bpmx
