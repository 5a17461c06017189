/*
 * trace_core_driver.cpp — runs csrc/bpmx_beats_core.h as plain C++ (the serial
 * executor) with the decision trace on, for tests/test_trace_core.py and as
 * the comparison target of tests/test_gpu_trace.py.  Host code only.
 *
 *   trace_core_driver IN OUT TRACE [stage]
 *
 * IN and OUT: beats_core_driver's formats (OUT is what the core gives with the
 * trace on, to be compared with that driver's, which runs it with the trace
 * off).
 * TRACE: per case
 *        int32 n_lt, double record[n][BPMX_TR_NFIELDS], int32 code[n],
 *        int32 lt_pos[n], double lt_bpm[n], double dev_t[n], double dev[n],
 *        int32 gap[n]
 * whole slices as the device keeps them: every byte the core did not write is
 * 0xFF, so a comparison of whole slices also compares what was left alone.
 *
 * Every array is its own allocation of exactly the size the core may touch
 * (dev_t / dev: n - 1 entries), so a sanitizer build reports any access
 * beyond it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_beats_core.h"

using namespace bpmx;

template <class T>
static T *make(size_t n) {
    const size_t b = n ? n * sizeof(T) : 1;
    T *p = (T *)std::malloc(b);
    std::memset(p, 0xFF, b);
    return p;
}
template <class T>
static bool get(FILE *f, T *p, size_t n) {
    return std::fread(p, sizeof(T), n, f) == n;
}
template <class T>
static bool put(FILE *f, const T *p, size_t n) {
    return std::fwrite(p, sizeof(T), n, f) == n;
}
/* m entries of p, then 0xFF up to n entries */
template <class T>
static bool put_padded(FILE *f, const T *p, size_t m, size_t n) {
    if (!put(f, p, m)) return false;
    T fill;
    std::memset(&fill, 0xFF, sizeof(T));
    for (size_t i = m; i < n; ++i)
        if (!put(f, &fill, 1)) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s IN OUT TRACE [stage]\n", argv[0]);
        return 2;
    }
    const bool stage = argc > 4 && std::strcmp(argv[4], "stage") == 0;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb"), *tro = std::fopen(argv[3], "wb");
    if (!in || !out || !tro) { std::perror("open"); return 2; }
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
        const size_t nd = n > 1 ? (size_t)n - 1 : 0;
        int32_t n_lt = -1;
        beats_trace tr;
        tr.rec = make<double>((size_t)n * BPMX_TR_NFIELDS);
        tr.code = make<int32_t>(n);
        tr.lt_pos = make<int32_t>(n);
        tr.lt_bpm = make<double>(n);
        tr.n_lt = &n_lt;
        tr.dev_t = make<double>(nd);
        tr.dev = make<double>(nd);
        tr.gap = make<int32_t>(n);
        const int32_t status = beats_core(beats_serial(), n, ip, ep, flo, sr, P, hint, w, fin, &n_final, bt, bv,
                                          &n_bpm, pass, tags, tr);
        if (n_final < 0 || n_final > n || n_bpm < 0 || n_bpm > n || n_lt < 0 || n_lt > n) return 4;
        if (!put(out, &status, 1) || !put(out, &n_final, 1) || !put(out, &n_bpm, 1) || !put(out, pass, 3) ||
            !put(out, fin, n_final) || !put(out, bt, n_bpm) || !put(out, bv, n_bpm) || !put(out, tags, n))
            return 5;
        if (!put(tro, &n_lt, 1) || !put(tro, tr.rec, (size_t)n * BPMX_TR_NFIELDS) || !put(tro, tr.code, n) ||
            !put(tro, tr.lt_pos, n) || !put(tro, tr.lt_bpm, n) || !put_padded(tro, tr.dev_t, nd, n) ||
            !put_padded(tro, tr.dev, nd, n) || !put(tro, tr.gap, n))
            return 5;
        std::free(idx); std::free(env); std::free(flo); std::free(ws);
        std::free(fin); std::free(bt); std::free(bv); std::free(tags);
        std::free(tr.rec); std::free(tr.code); std::free(tr.lt_pos); std::free(tr.lt_bpm);
        std::free(tr.dev_t); std::free(tr.dev); std::free(tr.gap);
    }
    std::fclose(in);
    std::fclose(tro);
    return std::fclose(out) == 0 ? 0 : 5;
}
