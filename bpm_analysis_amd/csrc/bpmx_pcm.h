/*
 * bpmx_pcm.h — the value of a PCM frame, for the kernels and for host drivers
 * (no HIP header: a plain C++ compiler takes it).
 */
#ifndef BPMX_PCM_H
#define BPMX_PCM_H

#include <stdint.h>

#include "../../include/bpmx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BPMX_HDI __host__ __device__ __forceinline__
#else
#define BPMX_HDI inline
#endif

namespace bpmx {

/* BPMX_DT_I24, stated once: a packed 24-bit element (3 bytes, little-endian,
 * two's complement, any byte alignment) IS the int32 sample v << 8, v its
 * sign-extended value: the array scipy.io.wavfile.read makes of the file.  So
 * an I24 batch behaves in every mode as the I32 batch of those samples: its
 * mono working dtype is int32 (odd extension and np.abs wrap in int32), its
 * channel mean the f64 mean of the int32 values. */
struct pcm24 {
    uint8_t b[3];
    BPMX_HDI operator int32_t() const {
        return (int32_t)((uint32_t)b[0] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 24);
    }
};
static_assert(sizeof(pcm24) == 3 && alignof(pcm24) == 1, "packed 24-bit element");

/* numpy dtype of x after `np.mean(axis=1)` (bpm_analysis.py:1015-1016):
 * mono keeps its dtype, multi-channel ints -> f64, f32 -> f32. */
BPMX_HDI int work_dtype(int dtype, int channels) {
    if (dtype == BPMX_DT_I24) dtype = BPMX_DT_I32;
    if (channels <= 1) return dtype;
    return dtype == BPMX_DT_F32 ? BPMX_DT_F32 : BPMX_DT_F64;
}

BPMX_HDI double load_pcm(const void *pcm, int dtype, int64_t idx) {
    switch (dtype) {
    case BPMX_DT_U8: return (double)((const uint8_t *)pcm)[idx];
    case BPMX_DT_I16: return (double)((const int16_t *)pcm)[idx];
    case BPMX_DT_I32: return (double)((const int32_t *)pcm)[idx];
    case BPMX_DT_F32: return (double)((const float *)pcm)[idx];
    case BPMX_DT_I24: return (double)(int32_t)((const pcm24 *)pcm)[idx];
    default: return ((const double *)pcm)[idx];
    }
}

/* value of frame `frame` after the channel mean */
BPMX_HDI double frame_value(const void *pcm, int dtype, int channels, int64_t frame) {
    if (channels <= 1) return load_pcm(pcm, dtype, frame);
    if (dtype == BPMX_DT_F32) {
        const float *p = (const float *)pcm + frame * channels;
        float s = p[0];
        for (int c = 1; c < channels; ++c) s = s + p[c];
        return (double)(s / (float)channels);
    }
    double s = load_pcm(pcm, dtype, frame * channels);
    for (int c = 1; c < channels; ++c) s = s + load_pcm(pcm, dtype, frame * channels + c);
    return s / (double)channels;
}

}  // namespace bpmx

#endif
