/*
 * k_pack.hip — bpmx_pack: a finished run's results in compact form, so a
 * batch consumer downloads what it reads instead of four sum(Nd)-long arrays.
 *
 *   k_pack_scan     per table (raw peaks, troughs) one workgroup: the exclusive
 *                   prefix sums of the per-file counts, tile after tile of
 *                   PK_SCAN_T files with a carry, so any number of files
 *   k_pack_gather   per (file, table) one workgroup: index, env and floor at
 *                   each peak / trough, copied as bit patterns; entries whose
 *                   table position is at or beyond the capacity are dropped
 *   k_pack_trough_floor  bpmx_pack_trough_floor: the floor at the packed
 *                   troughs, from the table's own offsets and indices
 *   k_pack_plot     bpmx_pack_plot: env and floor at every kf-th sample of each
 *                   file, per workgroup one chunk of kept entries; at kf = 1
 *                   16 bytes per lane where source and destination share
 *                   their 16-byte phase
 *   k_y16_max       per file max|y|: |y| bit patterns order as unsigned
 *                   integers and every NaN pattern lies above inf, so a 64-bit
 *                   atomic maximum of the bits propagates a NaN by itself
 *   k_y16_quant     the debug WAV's int16 samples (bpm_analysis.py:1057-1060):
 *                   trunc((y / m) * 32767), two rounded f64 operations (the
 *                   build has -ffp-contract=off); zeros when m is 0, NaN or inf
 */
#include "bpmx_common.h"
#include "bpmx_kernels.h"

namespace bpmx {

namespace {
typedef unsigned long long u64;
constexpr u64 ABS_MASK = 0x7fffffffffffffffull, INF_BITS = 0x7ff0000000000000ull, QNAN_BITS = 0x7ff8000000000000ull;

/* a file's count as every pack kernel takes it: never outside its slice */
__device__ __forceinline__ int64_t pack_count(int32_t n, int64_t nd) {
    const int64_t c = n < 0 ? 0 : (int64_t)n;
    return c < nd ? c : nd;
}
}  // namespace

__global__ __launch_bounds__(PK_SCAN_T) void k_pack_scan(PackArgs A) {
    const int w = blockIdx.x;
    if (!A.off[w]) return;
    constexpr int NW = PK_SCAN_T / 64;
    __shared__ long long wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t F = A.n_files;
    long long carry = 0;
    for (int64_t base = 0; base < F; base += PK_SCAN_T) {
        const int64_t f = base + tid;
        const long long c = f < F ? (long long)pack_count(A.cnt[w][f], A.doff[f + 1] - A.doff[f]) : 0;
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
        if (f < F) A.off[w][f] = carry + pre + v - c;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) A.off[w][F] = carry;
}

__global__ __launch_bounds__(PK_GATHER_T) void k_pack_gather(PackArgs A) {
    const int64_t f = blockIdx.x;
    const int w = blockIdx.y;
    if (!A.off[w]) return;
    const int64_t D = A.doff[f], nd = A.doff[f + 1] - D;
    const int64_t n = pack_count(A.cnt[w][f], nd), o = A.off[w][f], cap = A.cap[w];
    const u64 *env = (const u64 *)A.env + D;
    const u64 *flo = w == 0 ? (const u64 *)A.floor + D : nullptr;
    u64 *oenv = (u64 *)A.oenv[w], *oflo = w == 0 ? (u64 *)A.ofloor : nullptr;
    for (int64_t k = threadIdx.x; k < n; k += PK_GATHER_T) {
        const int64_t j = o + k;
        if (j >= cap) break;
        const int64_t i = A.idx[w][D + k];
        const bool in = i >= 0 && i < nd;      /* a run's indices always are; foreign input reads nothing outside */
        A.oidx[w][j] = (int32_t)i;
        oenv[j] = in ? env[i] : QNAN_BITS;
        if (oflo) oflo[j] = in ? flo[i] : QNAN_BITS;
    }
}

/* tr_floor[j] = floor[D_f + tr_idx[j]] as bit patterns, per file one
 * workgroup; the slice is clipped to the capacity, an index outside the
 * recording reads nothing */
__global__ __launch_bounds__(PK_GATHER_T) void k_pack_trough_floor(TroughFloorArgs A) {
    const int64_t f = blockIdx.x;
    const int64_t D = A.doff[f], nd = A.doff[f + 1] - D;
    const int64_t o = A.tr_off[f];
    int64_t e = A.tr_off[f + 1];
    if (o < 0) return;
    if (e > A.cap) e = A.cap;
    const u64 *flo = (const u64 *)A.floor + D;
    u64 *out = (u64 *)A.out;
    for (int64_t j = o + threadIdx.x; j < e; j += PK_GATHER_T) {
        const int64_t i = A.tr_idx[j];
        out[j] = (i >= 0 && i < nd) ? flo[i] : QNAN_BITS;
    }
}

/* dst[P_f + j] = src[D_f + j * kf] as bit patterns, j in this workgroup's chunk
 * of file f's kept entries (the host lists a workgroup per non-empty chunk, so
 * 1 <= m <= PK_PLOT_CHUNK).  Writes are contiguous 8 or 16 bytes per lane.  At
 * kf > 1 the reads are one 8-byte word per lane kf words apart: no word is
 * read twice, and up to kf = 8 a wave still uses every 64-byte line it
 * touches, beyond that a line per lane, which is what a strided gather costs
 * anywhere; the source is read once, so nothing is staged in LDS. */
__global__ __launch_bounds__(PK_PLOT_T) void k_pack_plot(PlotArgs A) {
    const int64_t F = A.n_files;
    const int64_t *doff = A.geo, *poff = doff + F + 1, *boff = poff + F + 1, *kfs = boff + F + 1, *bfile = kfs + F;
    const int64_t f = bfile[blockIdx.x];
    const int64_t kf = kfs[f];
    const int64_t j0 = ((int64_t)blockIdx.x - boff[f]) * PK_PLOT_CHUNK;
    int64_t m = poff[f + 1] - poff[f] - j0;
    if (m > PK_PLOT_CHUNK) m = PK_PLOT_CHUNK;
    if (m <= 0) return;
    const u64 *src = (const u64 *)A.src[blockIdx.y] + doff[f] + j0 * kf;
    u64 *dst = (u64 *)A.dst[blockIdx.y] + poff[f] + j0;
    const int t = threadIdx.x;
    if (kf == 1 && !(((uintptr_t)src ^ (uintptr_t)dst) & 8)) {
        /* a scalar head up to the first 16-byte boundary, pairs, a scalar tail */
        const int64_t lo = ((uintptr_t)dst & 8) ? 1 : 0;
        const int64_t npair = (m - lo) / 2;
        if (t == 0 && lo) dst[0] = src[0];
        if (t == 1 && lo + 2 * npair < m) dst[m - 1] = src[m - 1];
        const ulonglong2 *s2 = (const ulonglong2 *)(src + lo);
        ulonglong2 *d2 = (ulonglong2 *)(dst + lo);
        for (int64_t q = t; q < npair; q += PK_PLOT_T) d2[q] = s2[q];
    } else {
        for (int64_t j = t; j < m; j += PK_PLOT_T) dst[j] = src[j * kf];
    }
}

__global__ __launch_bounds__(PK_Y16_T) void k_y16_max(Y16Args A) {
    const int64_t f = blockIdx.x;
    const int64_t D = A.doff[f], nd = A.doff[f + 1] - D;
    const int64_t first = (int64_t)blockIdx.y * PK_Y16_T, stride = (int64_t)gridDim.y * PK_Y16_T;
    if (first >= nd) return;
    const u64 *y = (const u64 *)A.y + D;
    u64 m = 0;
    for (int64_t i = first + threadIdx.x; i < nd; i += stride) {
        const u64 b = y[i] & ABS_MASK;
        m = b > m ? b : m;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 t = __shfl_xor(m, d, 64);
        m = t > m ? t : m;
    }
    __shared__ u64 wm[PK_Y16_T / 64];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < PK_Y16_T / 64; ++k) m = wm[k] > m ? wm[k] : m;
        if (m) atomicMax(A.ymax + f, m);
    }
}

namespace {
__device__ __forceinline__ uint32_t y16_one(double v, double m, bool live) {
    if (!live) return 0;
    const double q = v / m;
    const double t = q * 32767.0;
    return (uint32_t)(uint16_t)(int16_t)(int32_t)t;
}
}  // namespace

__global__ __launch_bounds__(PK_Y16_T) void k_y16_quant(Y16Args A) {
    const int64_t f = blockIdx.x;
    const int64_t D = A.doff[f], nd = A.doff[f + 1] - D;
    if (nd <= 0) return;
    const u64 mb = A.ymax[f];
    const bool live = mb != 0 && mb < INF_BITS;
    const double m = __longlong_as_double((long long)mb);
    const double *y = A.y + D;
    int16_t *o = A.y16 + D;
    /* the slice is 2-byte aligned only: a scalar head up to the first 4-byte
     * boundary, pairs as one 32-bit store each, a scalar tail */
    const int64_t lo = ((uintptr_t)o & 2) ? 1 : 0;
    const int64_t npair = (nd - lo) / 2;
    if (blockIdx.y == 0) {
        if (threadIdx.x == 0 && lo) o[0] = (int16_t)y16_one(y[0], m, live);
        if (threadIdx.x == 1 && lo + 2 * npair < nd) o[nd - 1] = (int16_t)y16_one(y[nd - 1], m, live);
    }
    const int64_t stride = (int64_t)gridDim.y * PK_Y16_T;
    for (int64_t q = (int64_t)blockIdx.y * PK_Y16_T + threadIdx.x; q < npair; q += stride) {
        const int64_t i = lo + 2 * q;
        const uint32_t a = y16_one(y[i], m, live), b = y16_one(y[i + 1], m, live);
        *(uint32_t *)(o + i) = a | (b << 16);
    }
}

}  // namespace bpmx
