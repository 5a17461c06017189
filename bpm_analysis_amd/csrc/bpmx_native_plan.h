/*
 * bpmx_native_plan.h — native mode's block-kernel selection and tile sizes, as
 * pure host arithmetic: which of the k_native_blocks kernels a batch takes,
 * how many decimation blocks a tile holds, and which form k_native_carry's
 * tail and carry scan take.  k_envelope_native.hip launches by this plan;
 * tests/native_plan_driver.hip prints it without a GPU.
 */
#ifndef BPMX_NATIVE_PLAN_H
#define BPMX_NATIVE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bpmx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BPMX_NP_HD __host__ __device__
#else
#define BPMX_NP_HD
#endif

namespace bpmx {

constexpr int NAT_DSMAX = 1280;       /* decimation factors up to fs/300 - 1 at 384 kHz (tail buffers) */

/* k_native_carry's tail recursion, lane-parallel: the exact per-sample
 * recursion z' = A z + B u, y = C z + D u (SosStep, original basis) over the
 * nt <= NAT_TT_PAR tail samples as its impulse response, row m of the tail
 * table holding C A^m, A^m B, A^m zi and h_m (h_0 = D, h_m = C A^(m-1) B),
 * built on the host in long double from the same coefficients */
constexpr int NAT_TT_ROWS = NAT_DSMAX + 20, NAT_TT_PAR = 320;

constexpr int NAT_CPF = 8;      /* tiles per lane held in registers by k_native_carry */

constexpr int NAT_ET_SIZE = 45; /* doubles of the block kernels' epilogue constants in LDS (ET_SIZE) */

/* k_native_blocks_i16 and the generic kernel's staged stereo branch */
constexpr int NB_RCH = 20;              /* 16-byte chunks per lane per tile: <= 10240 samples */

/* k_native_blocks_mfma */
constexpr int NM_NDMA = 18;                      /* DMA wave-instructions per tile, always all issued, all lanes on */
constexpr int NM_SLOT_CH = NM_NDMA * 64;          /* 16-byte chunks per slot (18,432 B) */

/* blocks per tile the slot holds: every k of the last block's K steps (+2
 * samples for the odd-offset align) must stay inside the slot */
BPMX_NP_HD constexpr int nm_tile_blocks(int ds, int ks) {
    return ((NM_SLOT_CH * 8 - 7 - 32 * ks - 2) / ds + 1) < 64 ? ((NM_SLOT_CH * 8 - 7 - 32 * ks - 2) / ds + 1) : 64;
}

/* k_native_blocks_mfma24: packed 24-bit mono in the same slots, as bytes.
 * A tile's bytes start up to 15 past the slot's first (the DMA runs from the
 * 16-byte boundary below them); the last block's last K step reads 13 dwords
 * from the dword at or below its first byte, i.e. up to 3 * 32 ks + 4 bytes
 * from the block's start.  Rounded down to an even count: k_hilbert_env makes
 * yd of the full tiles itself only when a tile holds an even number of blocks */
BPMX_NP_HD constexpr int nm24_tile_blocks(int ds, int ks) {
    return ((NM_SLOT_CH * 16 - 15 - 96 * ks - 4) / (3 * ds) + 1) < 64
               ? ((NM_SLOT_CH * 16 - 15 - 96 * ks - 4) / (3 * ds) + 1) & ~1
               : 64;
}

/* k_native_blocks_mfma_big */
constexpr int NB_WAVES = 4, NB_SLOTS = 2, NB_NDMA = 19;   /* waves, slots per wave, DMA instructions (KiB) per slot */
BPMX_NP_HD inline int nb_sub_blocks(int ds, int ch, int ks64, int ndma) {
    const int hw = ndma * 64 * 8;                    /* halfwords per slot */
    const int b = (hw - 7 - 64 * ks64 - 2) / (ds * ch) + 1;
    return b < 16 ? b : 16;                          /* one 16-column N tile per sub-tile */
}

/* k_native_blocks_dma */
constexpr int ND_WAVES = 4;
constexpr int ND_LDS = 160 * 1024;

/* host: DMA wave-instructions per tile (1 KiB each) so that four slots, the
 * coefficient table and the epilogue constants fit the CU's LDS */
inline int nd_ndma(int ds) {
    const int coef = (ds + 1) * 64;
    const int n = (ND_LDS - coef - 1024) / (ND_WAVES * 1024);
    return n < 38 ? n : 38;
}
/* blocks per tile: the slot holds the <= 7-element alignment offset and
 * (bt ds + 1) frames of ch int16 elements; at most 32 (two lanes per block) */
inline int nd_tile_blocks(int ds, int ch) {
    const int n = nd_ndma(ds);
    if (n < 1) return 0;
    const int b = ((n * 64 * 8 - 7) / ch - 1) / ds;
    return b < 32 ? b : 32;
}
inline size_t nd_lds_bytes(int ds) {
    return (size_t)nd_ndma(ds) * ND_WAVES * 1024 + (size_t)(ds + 1) * 64 + NAT_ET_SIZE * 8;
}

/* the block kernel a batch takes */
enum {
    NAT_R_MFMA3 = 0,    /* k_native_blocks_mfma<3>: int16 mono, ds + 1 <= 96 */
    NAT_R_MFMA5,        /* k_native_blocks_mfma<5>: int16 mono, ds + 1 <= 160 */
    NAT_R_BIG5,         /* k_native_blocks_mfma_big<5>: int16, channels x (ds + 1) <= 320 */
    NAT_R_BIG10,        /* k_native_blocks_mfma_big<10>: <= 640 */
    NAT_R_DMA1,         /* k_native_blocks_dma<1>: int16 mono on request */
    NAT_R_DMA2,         /* k_native_blocks_dma<2>: the rest of int16 stereo */
    NAT_R_I16,          /* k_native_blocks_i16: int16 mono, f64 VALU */
    NAT_R_GEN,          /* k_native_blocks_gen<dtype, multi> */
    NAT_R_M24_3,        /* k_native_blocks_mfma24<3>: packed 24-bit mono, ds + 1 <= 96 */
    NAT_R_M24_5         /* k_native_blocks_mfma24<5>: packed 24-bit mono, ds + 1 <= 160 */
};

struct NativePlan {
    int route;
    int gen_dtype;              /* NAT_R_GEN: the instantiation, */
    bool gen_multi;             /* and whether its LDS-staged int16 stereo branch applies */
    bool gen_staged;
    int mfma_ks;                /* K steps of 32 the matrix-core tables are built for (0: none; also off that route) */
    int big_ks, big_bs;         /* big-K kernel: K steps of 64 (0: K too large), blocks per sub-tile */
    int ndma;                   /* NAT_R_DMA*: DMA wave-instructions per tile */
    int bt;                     /* blocks per full tile */
    int64_t gstr;               /* gamma row per tile, in doubles */
    size_t lds;                 /* dynamic LDS bytes of the launch */
    int64_t key15, key16;       /* what the table cache key holds beyond the coefficients and ds */
};

/* dtype, channels, ds and options are the run's; align is the PCM address
 * mod 16; total the batch's elements (frames x channels).  BPMX_E_LIMIT
 * beyond NAT_DSMAX. */
inline int native_block_plan(int dtype, int channels, int ds, int32_t options, unsigned align, int64_t total,
                             NativePlan *out) {
    NativePlan &N = *out;
    N = NativePlan{};
    if (ds > NAT_DSMAX) return BPMX_E_LIMIT;
    /* matrix-core path: int16 mono, ds + 1 <= 160 (KS K steps of 32 samples) */
    N.mfma_ks = ds + 1 <= 96 ? 3 : (ds + 1 <= 160 ? 5 : 0);
    const bool aligned16 = (align & 15) == 0;
    const bool i16_fast = dtype == BPMX_DT_I16 && aligned16 && total >= 16 &&
                          !(options & (BPMX_OPT_NATIVE_F64 | BPMX_OPT_NATIVE_DMA));
    const bool use_mfma = N.mfma_ks && i16_fast && channels == 1;
    /* int16 mono beyond K = 160 and int16 stereo: the big-K matrix-core kernel
     * (K = channels x (ds + 1) <= 640, K steps of 64) */
    const int kbig = channels * (ds + 1);
    N.big_ks = kbig <= 320 ? 5 : (kbig <= 640 ? 10 : 0);
    N.big_bs = N.big_ks ? nb_sub_blocks(ds, channels, N.big_ks, NB_NDMA) : 0;
    const bool use_big = !use_mfma && i16_fast && N.big_ks && (channels == 1 || channels == 2) && N.big_bs >= 1;
    /* the rest of int16 stereo (and, on request, mono) through the LDS-DMA f64 kernel */
    const bool use_dma = !use_mfma && !use_big && dtype == BPMX_DT_I16 && aligned16 && total >= 16 &&
                         (channels == 2 || (channels == 1 && (options & BPMX_OPT_NATIVE_DMA))) &&
                         !(options & BPMX_OPT_NATIVE_F64) && nd_tile_blocks(ds, channels) >= 1;
    const bool fast = dtype == BPMX_DT_I16 && channels == 1 && aligned16;
    /* packed 24-bit mono on the matrix cores, at any byte alignment (its DMA
     * starts at the 16-byte boundary below each tile); total >= 16: anything
     * shorter holds no active recording and not always a whole 16-byte chunk */
    const bool use_m24 = dtype == BPMX_DT_I24 && channels == 1 && N.mfma_ks && total >= 16 &&
                         !(options & BPMX_OPT_NATIVE_F64);
    /* tiles of bt blocks: the LDS tile (slot) must hold the tile's samples;
     * the int16 path's LDS tile holds <= NB_RCH*512 samples */
    const int bt_gen = (NB_RCH * 512 - 16) / ds < 64 ? (NB_RCH * 512 - 16) / ds : 64;
    if (use_mfma) {
        N.route = N.mfma_ks == 3 ? NAT_R_MFMA3 : NAT_R_MFMA5;
        N.bt = nm_tile_blocks(ds, N.mfma_ks);
    } else if (use_m24) {
        N.route = N.mfma_ks == 3 ? NAT_R_M24_3 : NAT_R_M24_5;
        N.bt = nm24_tile_blocks(ds, N.mfma_ks);
    } else if (use_big) {
        N.route = N.big_ks == 5 ? NAT_R_BIG5 : NAT_R_BIG10;
        N.bt = N.big_bs * (64 / N.big_bs);
        N.lds = (size_t)NB_SLOTS * NB_NDMA * NB_WAVES * 1024;
    } else if (use_dma) {
        N.route = channels == 2 ? NAT_R_DMA2 : NAT_R_DMA1;
        N.bt = nd_tile_blocks(ds, channels);
        N.ndma = nd_ndma(ds);
        N.lds = nd_lds_bytes(ds);
    } else if (fast) {
        N.route = NAT_R_I16;
        N.bt = bt_gen;
    } else {
        N.route = NAT_R_GEN;
        N.bt = bt_gen;
        N.gen_dtype = (dtype >= BPMX_DT_U8 && dtype <= BPMX_DT_F32) || dtype == BPMX_DT_I24 ? dtype : BPMX_DT_F64;
        N.gen_multi = channels > 1;
        N.gen_staged = dtype == BPMX_DT_I16 && channels == 2 && (align & 3) == 0;
    }
    N.gstr = (N.bt + 15) / 16 * 16;
    N.key15 = N.bt;
    N.key16 = use_big ? 1000 * channels + N.big_ks : (use_m24 ? 24 : 0);   /* the 24-bit tables differ from int16's */
    return BPMX_OK;
}

/* k_native_carry's tail of a recording of n frames: the samples from the last
 * decimated one on plus the 15 of the right pad; lane-parallel up to
 * NAT_TT_PAR of them, else the serial recursion on lane 0 */
inline int64_t nat_tail_len(int64_t n, int ds) {
    const int64_t nd = (n + ds - 1) / ds;
    return n - (nd - 1) * ds + 15;
}
inline bool nat_tail_parallel(int64_t n, int ds) { return nat_tail_len(n, ds) <= NAT_TT_PAR; }

/* k_native_carry's scan over a recording's full tiles: each lane's run of
 * tiles in registers up to NAT_CPF tiles per lane, else in chunks */
inline bool nat_carry_chunked(int64_t n, int ds, int bt) {
    const int64_t nd = (n + ds - 1) / ds, tf = (nd - 1) / bt;
    return (tf + 63) / 64 > NAT_CPF;
}

}  // namespace bpmx

#endif
