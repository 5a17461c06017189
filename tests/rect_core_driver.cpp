/* Host driver for csrc/bpmx_rect_core.h: the rectified-mode envelope's
 * arithmetic as plain C++ (tests/test_rect_core.py).
 *
 *   rect_core_driver cases.bin out.bin
 *
 * cases.bin: int32 count, then per case int32 dtype, channels, window, pad,
 * int64 frames, and the interleaved samples.  out.bin: per case int32
 * has_exact, pad, `frames` doubles by the pandas recursion (rect_value,
 * rect_roll_mean), and when the exact-integer route applies `frames` doubles
 * by it (rect_int_frame prefix sums, rect_mean_exact). */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_rect_core.h"

using namespace bpmx;

static size_t dt_bytes(int dt) { return dt == BPMX_DT_U8 ? 1 : dt == BPMX_DT_I16 ? 2 : dt == BPMX_DT_F64 ? 8 : 4; }

template <typename T>
static void exact(int dt, bool stereo, const void *pcm, int64_t n, int64_t w, std::vector<double> &out) {
    const T *p = (const T *)pcm;
    std::vector<int64_t> P((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; ++j) P[j + 1] = P[j] + rect_int_frame<T>(dt, stereo, p + j * (stereo ? 2 : 1));
    for (int64_t i = 0; i < n; ++i) {
        int64_t s, e;
        win_bounds(i, n, w, s, e);
        out[(size_t)i] = rect_mean_exact(P[e] - P[s], e - s, stereo);
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *outf = std::fopen(argv[2], "wb");
    if (!in || !outf) return 2;
    int32_t count = 0;
    if (std::fread(&count, 4, 1, in) != 1) return 3;
    for (int32_t c = 0; c < count; ++c) {
        int32_t h[4];
        int64_t n;
        if (std::fread(h, 4, 4, in) != 4 || std::fread(&n, 8, 1, in) != 1) return 3;
        const int dt = h[0], ch = h[1];
        const int64_t w = h[2];
        std::vector<unsigned char> raw((size_t)n * ch * dt_bytes(dt) + 8);
        const size_t nb = (size_t)n * ch * dt_bytes(dt);
        if (nb && std::fread(raw.data(), 1, nb, in) != nb) return 3;
        /* an exact-size copy, so that the sanitizer sees a read past the samples */
        std::vector<unsigned char> pcm(raw.begin(), raw.begin() + nb);
        std::vector<double> gen((size_t)n), ex((size_t)n);
        rect_roll_mean(n, w, [&](int64_t j) { return rect_value(pcm.data(), dt, ch, j); },
                       [&](int64_t i, double m) { gen[(size_t)i] = m; });
        const bool has_exact = dt <= BPMX_DT_I32 && ch <= 2 && w <= RECT_W_EXACT_MAX;
        if (has_exact) {
            if (dt == BPMX_DT_U8) exact<uint8_t>(dt, ch == 2, pcm.data(), n, w, ex);
            else if (dt == BPMX_DT_I16) exact<int16_t>(dt, ch == 2, pcm.data(), n, w, ex);
            else exact<int32_t>(dt, ch == 2, pcm.data(), n, w, ex);
        }
        const int32_t oh[2] = {has_exact ? 1 : 0, 0};
        std::fwrite(oh, 4, 2, outf);
        std::fwrite(gen.data(), 8, (size_t)n, outf);
        if (has_exact) std::fwrite(ex.data(), 8, (size_t)n, outf);
    }
    std::fclose(in);
    return std::fclose(outf) == 0 ? 0 : 4;
}
