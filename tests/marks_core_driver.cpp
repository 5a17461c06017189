/*
 * marks_core_driver.cpp — runs csrc/bpmx_marks_core.h as plain C++ for
 * tests/test_marks_core.py.  Host code only.
 *
 *   marks_core_driver IN OUT [LANES]   the cases of IN; LANES > 1: that many threads as the lanes of one
 *                                      workgroup, sync() a barrier (the kernel's partition of the work)
 *
 * IN:  int32 n_cases, then per case
 *        int32 nr, int32 sr, int64 nd (-1: none), double window_sec, int32 rf_ms[nr], int32 rf_type[nr]
 * OUT: per case
 *        int32 status, int32 record[8], int32 n, int32 idx[n], int8 tag[n], int32 gap[n], double env[n],
 *        double floor[n], int32 n_final, int32 final[n_final], int32 n_bpm, double bpm_t[n_bpm],
 *        double bpm[n_bpm], double pass[3]
 *
 * Every array is its own allocation of exactly its entries (the scratch of nr
 * marks, the outputs of n rows, the workspace of marks_ws_bytes(n_s1, LANES)),
 * so a sanitizer build reports any access beyond them.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_marks_core.h"

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

/* the lanes of one workgroup as threads */
struct barrier {
    std::mutex m;
    std::condition_variable cv;
    int width, waiting = 0;
    long round = 0;
    explicit barrier(int w) : width(w) {}
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const long r = round;
        if (++waiting == width) {
            waiting = 0;
            ++round;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return round != r; });
        }
    }
};
struct lanes_exec {
    int l, w;
    barrier *b;
    int lane() const { return l; }
    int width() const { return w; }
    void sync() const { if (w > 1) b->wait(); }
};

template <class F>
static void run(int lanes, F body) {
    std::vector<std::thread> pool;
    for (int l = 1; l < lanes; ++l) pool.emplace_back(body, l);
    body(0);
    for (auto &t : pool) t.join();
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT [LANES]\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    const int lanes = argc > 3 ? std::atoi(argv[3]) : 1;
    if (lanes < 1 || lanes > 64) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t nr = 0, sr = 0;
        int64_t nd = -1;
        double window = 0;
        if (!get(in, &nr, 1) || !get(in, &sr, 1) || !get(in, &nd, 1) || !get(in, &window, 1) || nr < 0) return 3;
        int32_t *rm = make<int32_t>(nr), *rt = make<int32_t>(nr);
        if (!get(in, rm, nr) || !get(in, rt, nr)) return 3;
        void *hd = std::malloc(marks_ws_head(lanes));
        const marks_head h = marks_head_layout(hd, lanes);
        int32_t *k_idx = make<int32_t>(nr), *r_idx = make<int32_t>(nr);
        int8_t *k_type = make<int8_t>(nr), *r_tag = make<int8_t>(nr);
        int32_t cnt[MC_PER_FILE];
        barrier bar(lanes);
        run(lanes, [&](int l) {
            marks_rows(lanes_exec{l, lanes, &bar}, nr, rm, rt, sr, nd, h, k_idx, k_type, r_idx, r_tag, cnt);
        });
        const int32_t n = cnt[BPMX_MK_N_ROWS], ns1 = cnt[BPMX_MK_N_S1];
        if (n < 0 || n > nr || ns1 < 0 || ns1 > n) return 4;
        void *ws = std::malloc(beats_ws_bytes(ns1, false));
        const beats_ws w = beats_ws_layout(ws, ns1, false);
        marks_io io;
        io.pk_idx = make<int32_t>(n); io.pk_env = make<double>(n); io.pk_floor = make<double>(n);
        io.tags = make<int8_t>(n); io.gap = make<int32_t>(n);
        io.final_idx = make<int32_t>(ns1); io.bpm_t = make<double>(ns1); io.bpm = make<double>(ns1);
        int32_t n_final = -1, n_bpm = -1, record[BPMX_MARKS_RECORD], status = 0;
        double pass[3];
        io.n_final = &n_final; io.n_bpm = &n_bpm; io.pass = pass; io.record = record;
        run(lanes, [&](int l) {
            const int rc = marks_finish(lanes_exec{l, lanes, &bar}, n, r_idx, r_tag, cnt, sr, window, h, w, io);
            if (l == 0) status = rc;
        });
        if (n_final < 0 || n_final > ns1 || n_bpm < 0 || n_bpm > ns1) return 4;
        if (!put(out, &status, 1) || !put(out, record, BPMX_MARKS_RECORD) || !put(out, &n, 1) ||
            !put(out, io.pk_idx, n) || !put(out, io.tags, n) || !put(out, io.gap, n) || !put(out, io.pk_env, n) ||
            !put(out, io.pk_floor, n) || !put(out, &n_final, 1) || !put(out, io.final_idx, n_final) ||
            !put(out, &n_bpm, 1) || !put(out, io.bpm_t, n_bpm) || !put(out, io.bpm, n_bpm) || !put(out, pass, 3))
            return 5;
        std::free(rm); std::free(rt); std::free(hd); std::free(k_idx); std::free(r_idx); std::free(k_type);
        std::free(r_tag); std::free(ws);
        std::free(io.pk_idx); std::free(io.pk_env); std::free(io.pk_floor); std::free(io.tags); std::free(io.gap);
        std::free(io.final_idx); std::free(io.bpm_t); std::free(io.bpm);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
