/*
 * score_core_driver.cpp — runs csrc/bpmx_score_core.h as plain C++ for
 * tests/test_score_core.py.  Host code only.
 *
 *   score_core_driver IN OUT [LANES]   the cases of IN; LANES > 1: that many threads as the lanes of one
 *                                      workgroup, sync() a barrier (the kernel's partition of the work)
 *   score_core_driver ms OUT SR..      sc_ms(lb_round3(idx / sr)) for idx in [0, 4096) at every SR, as int32
 *
 * IN:  int32 n_cases, then per case
 *        int32 nd, int32 nr, int32 tol_ms, int32 gap_ms, int32 labelled,
 *        double lb_time[nd], int32 lb_type[nd], int32 rf_ms[nr], int32 rf_type[nr]
 * OUT: per case
 *        int32 status, int64 record[20], int32 nd, int32 nr (0, 0 where the core writes no rows),
 *        int32 sc_kind, sc_ref [nd], int32 rf_kind, rf_det [nr]
 *
 * Every array is its own allocation of exactly its entries, and the workspace
 * of exactly score_ws_bytes(nd, nr, LANES), so a sanitizer build reports any
 * access beyond them.  labelled = 0 gives the empty detected list and the
 * BPMX_SCORE_NO_LABELS bit, as in the kernel.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_labels_core.h"
#include "../bpm_analysis_amd/csrc/bpmx_score_core.h"

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

static int ms_table(int argc, char **argv) {
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror("open"); return 2; }
    for (int a = 3; a < argc; ++a) {
        const int32_t sr = std::atoi(argv[a]);
        for (int32_t i = 0; i < 4096; ++i) {
            const int32_t v = sc_ms(lb_round3((double)i / (double)sr));
            if (!put(out, &v, 1)) return 5;
        }
    }
    return std::fclose(out) == 0 ? 0 : 5;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT [LANES] | ms OUT SR...\n", argv[0]);
        return 2;
    }
    if (std::strcmp(argv[1], "ms") == 0) return ms_table(argc, argv);
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    const int lanes = argc > 3 ? std::atoi(argv[3]) : 1;
    if (lanes < 1 || lanes > 64) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t nd = 0, nr = 0, labelled = 0;
        bpmx_score_params P;
        if (!get(in, &nd, 1) || !get(in, &nr, 1) || !get(in, &P.tol_ms, 1) || !get(in, &P.gap_ms, 1) ||
            !get(in, &labelled, 1) || nd < 0 || nr < 0)
            return 3;
        double *lt = make<double>(nd);
        int32_t *ty = make<int32_t>(nd), *rm = make<int32_t>(nr), *rt = make<int32_t>(nr);
        if (!get(in, lt, nd) || !get(in, ty, nd) || !get(in, rm, nr) || !get(in, rt, nr)) return 3;
        const int32_t n = labelled ? nd : 0;
        void *ws = std::malloc(score_ws_bytes(n, nr, lanes));
        const score_ws w = score_ws_layout(ws, n, nr, lanes);
        score_io io;
        io.sc_kind = make<int32_t>(n); io.sc_ref = make<int32_t>(n);
        io.rf_kind = make<int32_t>(nr); io.rf_det = make<int32_t>(nr);
        int64_t record[BPMX_SCORE_RECORD];
        io.record = record;
        int32_t status = 0;
        barrier bar(lanes);
        std::vector<std::thread> pool;
        auto body = [&](int l) {
            const int rc = score_core(lanes_exec{l, lanes, &bar}, n, lt, ty, nr, rm, rt, P, w, io);
            if (l == 0) status = rc == BPMX_SCORE_OK && !labelled ? (int)BPMX_SCORE_NO_LABELS : rc;
        };
        for (int l = 1; l < lanes; ++l) pool.emplace_back(body, l);
        body(0);
        for (auto &t : pool) t.join();
        const int32_t od = status >= 0 ? n : 0, orf = status >= 0 ? nr : 0;
        if (!put(out, &status, 1) || !put(out, record, BPMX_SCORE_RECORD) || !put(out, &od, 1) || !put(out, &orf, 1) ||
            !put(out, io.sc_kind, od) || !put(out, io.sc_ref, od) || !put(out, io.rf_kind, orf) ||
            !put(out, io.rf_det, orf))
            return 5;
        std::free(lt); std::free(ty); std::free(rm); std::free(rt); std::free(ws);
        std::free(io.sc_kind); std::free(io.sc_ref); std::free(io.rf_kind); std::free(io.rf_det);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
