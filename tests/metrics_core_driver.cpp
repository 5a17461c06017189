/*
 * metrics_core_driver.cpp — runs csrc/bpmx_metrics_core.h as plain C++ (the
 * serial executor) for tests/test_metrics_core.py.  Host code only.
 *
 *   metrics_core_driver IN OUT [stage]
 *
 * IN:  int32 n_cases, then per case
 *        int32 nf, int32 m, int32 sr, int32 beats_status, int64 epoch_us,
 *        bpmx_metric_params, int32 final[nf] (samples), double bpm_t[m], double bpm[m]
 * OUT: per case
 *        int32 status, int32 n_hrv, int32 n_inc, int32 n_dec, double record[16],
 *        double hrv_time / rmssdc / sdnn / bpm [n_hrv] each,
 *        int32 inc_a[n_inc], inc_b[n_inc], double inc_slope[n_inc], inc_dur[n_inc], the same for dec
 *
 * Every array is its own allocation of exactly nf entries (what a file's
 * slice holds at least), so a sanitizer build reports any access beyond it.
 * `stage`: the workspace layout with the staged copies of the curve and the
 * beats in front (the form the GPU kernel keeps in LDS).  A beats status
 * other than 0 gives BPMX_METRICS_NONE as in the kernel.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bpm_analysis_amd/csrc/bpmx_metrics_core.h"

using namespace bpmx;

template <class T>
static T *make(size_t n) {
    return (T *)std::malloc(n ? n * sizeof(T) : 1);
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
        int32_t nf = 0, m = 0, sr = 0, bst = 0;
        int64_t epoch_us = 0;
        bpmx_metric_params P;
        if (!get(in, &nf, 1) || !get(in, &m, 1) || !get(in, &sr, 1) || !get(in, &bst, 1) || !get(in, &epoch_us, 1) ||
            !get(in, &P, 1) || nf < 0 || m < 0 || (m > 0 && m >= nf))
            return 3;
        int32_t *fin = make<int32_t>(nf);
        double *bt = make<double>(m), *bv = make<double>(m);
        if (!get(in, fin, nf) || !get(in, bt, m) || !get(in, bv, m)) return 3;
        const int fw = pw_frames(P.hrv_window_size_beats);
        void *ws = std::malloc(metrics_ws_bytes(nf, 1, fw, stage));
        const metrics_ws w = metrics_ws_layout(ws, nf, 1, fw, stage);
        const int32_t *fp = fin;
        const double *vp = bv;
        if (stage) {
            std::memcpy(w.fin_stage, fin, (size_t)nf * 4);
            std::memcpy(w.v_stage, bv, (size_t)m * 8);
            fp = w.fin_stage;
            vp = w.v_stage;
        }
        metrics_io io;
        io.hrv_time = make<double>(nf); io.hrv_rmssdc = make<double>(nf);
        io.hrv_sdnn = make<double>(nf); io.hrv_bpm = make<double>(nf);
        io.inc_a = make<int32_t>(nf); io.inc_b = make<int32_t>(nf);
        io.dec_a = make<int32_t>(nf); io.dec_b = make<int32_t>(nf);
        io.inc_slope = make<double>(nf); io.inc_dur = make<double>(nf);
        io.dec_slope = make<double>(nf); io.dec_dur = make<double>(nf);
        int32_t n_hrv = -1, n_inc = -1, n_dec = -1;
        double record[BPMX_METRICS_RECORD];
        io.n_hrv = &n_hrv; io.n_inc = &n_inc; io.n_dec = &n_dec; io.record = record;
        const int32_t status = metrics_core(beats_serial(), bst == 0 ? nf : 0, fp, bst == 0 ? m : 0, bt, vp, sr, P,
                                            epoch_us, w, io);
        if (n_hrv < 0 || n_hrv > nf || n_inc < 0 || n_inc > nf || n_dec < 0 || n_dec > nf) return 4;
        if (!put(out, &status, 1) || !put(out, &n_hrv, 1) || !put(out, &n_inc, 1) || !put(out, &n_dec, 1) ||
            !put(out, record, BPMX_METRICS_RECORD) || !put(out, io.hrv_time, n_hrv) ||
            !put(out, io.hrv_rmssdc, n_hrv) || !put(out, io.hrv_sdnn, n_hrv) || !put(out, io.hrv_bpm, n_hrv) ||
            !put(out, io.inc_a, n_inc) || !put(out, io.inc_b, n_inc) || !put(out, io.inc_slope, n_inc) ||
            !put(out, io.inc_dur, n_inc) || !put(out, io.dec_a, n_dec) || !put(out, io.dec_b, n_dec) ||
            !put(out, io.dec_slope, n_dec) || !put(out, io.dec_dur, n_dec))
            return 5;
        std::free(fin); std::free(bt); std::free(bv); std::free(ws);
        std::free(io.hrv_time); std::free(io.hrv_rmssdc); std::free(io.hrv_sdnn); std::free(io.hrv_bpm);
        std::free(io.inc_a); std::free(io.inc_b); std::free(io.dec_a); std::free(io.dec_b);
        std::free(io.inc_slope); std::free(io.inc_dur); std::free(io.dec_slope); std::free(io.dec_dur);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
