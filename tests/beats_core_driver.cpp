/*
 * beats_core_driver.cpp — runs csrc/bpmx_beats_core.h as plain C++ (the serial
 * executor) for tests/test_beats_core.py.  Host code only.
 *
 *   beats_core_driver IN OUT [stage]
 *
 * IN:  int32 n_cases, then per case
 *        int32 n, int32 sr, double hint (NaN = None), bpmx_beat_params,
 *        int32 idx[n], double env_pk[n], double floor_pk[n]
 * OUT: per case
 *        int32 status, int32 n_final, int32 n_bpm, double pass[3],
 *        int32 final[n_final], double bpm_t[n_bpm], double bpm[n_bpm], int8 tags[n]
 *
 * Every array is its own allocation of exactly the size the core may touch, so
 * a sanitizer build reports any access beyond it.  `stage`: the workspace
 * layout with the staged copies of idx and env_pk in front (the form the GPU
 * kernel keeps in LDS).
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_beats_core.h"

using namespace bpmx;

template <class T>
static T *make(size_t n) {
    return (T *)std::malloc(n * sizeof(T) ? n * sizeof(T) : 1);
}
template <class T>
static bool get(FILE *f, T *p, size_t n) {
    return std::fread(p, sizeof(T), n, f) == n;
}
template <class T>
static bool put(FILE *f, const T *p, size_t n) {
    return std::fwrite(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT [stage]\n", argv[0]);
        return 2;
    }
    const bool stage = argc > 3 && std::strcmp(argv[3], "stage") == 0;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t n = 0, sr = 0;
        double hint = 0;
        bpmx_beat_params P;
        if (!get(in, &n, 1) || !get(in, &sr, 1) || !get(in, &hint, 1) || !get(in, &P, 1) || n < 0) return 3;
        int32_t *idx = make<int32_t>(n);
        double *env = make<double>(n), *flo = make<double>(n);
        if (!get(in, idx, n) || !get(in, env, n) || !get(in, flo, n)) return 3;
        void *ws = std::malloc(beats_ws_bytes(n, stage));
        const beats_ws w = beats_ws_layout(ws, n, stage);
        const int32_t *ip = idx;
        const double *ep = env;
        if (stage) {
            std::memcpy(w.idx_stage, idx, (size_t)n * 4);
            std::memcpy(w.env_stage, env, (size_t)n * 8);
            ip = w.idx_stage;
            ep = w.env_stage;
        }
        int32_t *fin = make<int32_t>(n), n_final = -1, n_bpm = -1;
        double *bt = make<double>(n), *bv = make<double>(n), pass[3] = {0, 0, 0};
        int8_t *tags = make<int8_t>(n);
        const int32_t status = beats_core(beats_serial(), n, ip, ep, flo, sr, P, hint, w, fin, &n_final, bt, bv,
                                          &n_bpm, pass, tags);
        if (n_final < 0 || n_final > n || n_bpm < 0 || n_bpm > n) return 4;
        if (!put(out, &status, 1) || !put(out, &n_final, 1) || !put(out, &n_bpm, 1) || !put(out, pass, 3) ||
            !put(out, fin, n_final) || !put(out, bt, n_bpm) || !put(out, bv, n_bpm) || !put(out, tags, n))
            return 5;
        std::free(idx); std::free(env); std::free(flo); std::free(ws);
        std::free(fin); std::free(bt); std::free(bv); std::free(tags);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
