/*
 * labels_core_driver.cpp — runs csrc/bpmx_labels_core.h as plain C++ (the
 * serial executor) for tests/test_labels_core.py.  Host code only.
 *
 *   labels_core_driver IN OUT [LANES]  the cases of IN; LANES > 1: that many threads as the lanes of one
 *                                      workgroup, sync() a barrier (the kernel's partition of the work)
 *   labels_core_driver round OUT SR..  lb_round3(idx / sr) for idx in [0, 4096) at every SR, as doubles
 *
 * IN:  int32 n_cases, then per case
 *        int32 n, int32 nf, int32 m, int32 sr, int32 beats_status, double gap_sec,
 *        int32 idx[n], int8 tags[n], int32 gap[n], int32 final[nf] (samples), double bpm_t[m], double bpm[m]
 * OUT: per case
 *        int32 status, int32 n_labels, int32 n_pairs, int32 n_groups, double record[4],
 *        int32 lb_pos, lb_type [n_labels], double lb_time, lb_bpm [n_labels],
 *        int32 pr_s1, pr_s2 [n_pairs], double pr_dt [n_pairs],
 *        int32 gr_id, gr_first, gr_last, gr_s1, gr_pairs [n_groups], double gr_dt, gr_bpm [n_groups]
 *
 * Every array is its own allocation of exactly n entries (what a file's slice
 * holds), and the workspace of exactly labels_ws_bytes(n, LANES), so a sanitizer
 * build reports any access beyond them.  A beats status other than 0, or a
 * curve of as many rows as beats, gives BPMX_LABELS_NONE as in the kernel.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_labels_core.h"

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

static int round_table(int argc, char **argv) {
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror("open"); return 2; }
    for (int a = 3; a < argc; ++a) {
        const int32_t sr = std::atoi(argv[a]);
        for (int32_t i = 0; i < 4096; ++i) {
            const double v = lb_round3((double)i / (double)sr);
            if (!put(out, &v, 1)) return 5;
        }
    }
    return std::fclose(out) == 0 ? 0 : 5;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT | round OUT SR...\n", argv[0]);
        return 2;
    }
    if (std::strcmp(argv[1], "round") == 0) return round_table(argc, argv);
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    const int lanes = argc > 3 ? std::atoi(argv[3]) : 1;
    if (lanes < 1 || lanes > 64) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t n = 0, nf = 0, m = 0, sr = 0, bst = 0;
        bpmx_label_params P;
        if (!get(in, &n, 1) || !get(in, &nf, 1) || !get(in, &m, 1) || !get(in, &sr, 1) || !get(in, &bst, 1) ||
            !get(in, &P.gap_sec, 1) || n < 0 || nf < 0 || nf > n || m < 0)
            return 3;
        if (m > 0 && m >= nf) bst = -1;               /* a curve its beats cannot have: no labels, as in the kernel */
        int32_t *idx = make<int32_t>(n), *gap = make<int32_t>(n), *fin = make<int32_t>(nf);
        int8_t *tags = make<int8_t>(n);
        double *bt = make<double>(m), *bv = make<double>(m);
        if (!get(in, idx, n) || !get(in, tags, n) || !get(in, gap, n) || !get(in, fin, nf) || !get(in, bt, m) ||
            !get(in, bv, m))
            return 3;
        void *ws = std::malloc(labels_ws_bytes(n, lanes));
        const labels_ws w = labels_ws_layout(ws, n, lanes);
        labels_io io;
        io.lb_pos = make<int32_t>(n); io.lb_type = make<int32_t>(n);
        io.lb_time = make<double>(n); io.lb_bpm = make<double>(n);
        io.pr_s1 = make<int32_t>(n); io.pr_s2 = make<int32_t>(n); io.pr_dt = make<double>(n);
        io.gr_id = make<int32_t>(n); io.gr_first = make<int32_t>(n); io.gr_last = make<int32_t>(n);
        io.gr_s1 = make<int32_t>(n); io.gr_pairs = make<int32_t>(n);
        io.gr_dt = make<double>(n); io.gr_bpm = make<double>(n);
        int32_t nl = -1, np = -1, ng = -1;
        double record[BPMX_LABELS_RECORD];
        io.n_labels = &nl; io.n_pairs = &np; io.n_groups = &ng; io.record = record;
        int32_t status = 0;
        barrier bar(lanes);
        std::vector<std::thread> pool;
        auto body = [&](int l) {
            const int rc = labels_core(lanes_exec{l, lanes, &bar}, n, idx, tags, gap, bst == 0 ? nf : 0, fin,
                                       bst == 0 ? m : 0, bt, bv, sr, P, w, io);
            if (l == 0) status = rc;
        };
        for (int l = 1; l < lanes; ++l) pool.emplace_back(body, l);
        body(0);
        for (auto &t : pool) t.join();
        if (nl < 0 || nl > n || np < 0 || np > n || ng < 0 || ng > n) return 4;
        if (!put(out, &status, 1) || !put(out, &nl, 1) || !put(out, &np, 1) || !put(out, &ng, 1) ||
            !put(out, record, BPMX_LABELS_RECORD) || !put(out, io.lb_pos, nl) || !put(out, io.lb_type, nl) ||
            !put(out, io.lb_time, nl) || !put(out, io.lb_bpm, nl) || !put(out, io.pr_s1, np) ||
            !put(out, io.pr_s2, np) || !put(out, io.pr_dt, np) || !put(out, io.gr_id, ng) ||
            !put(out, io.gr_first, ng) || !put(out, io.gr_last, ng) || !put(out, io.gr_s1, ng) ||
            !put(out, io.gr_pairs, ng) || !put(out, io.gr_dt, ng) || !put(out, io.gr_bpm, ng))
            return 5;
        std::free(idx); std::free(gap); std::free(fin); std::free(tags); std::free(bt); std::free(bv); std::free(ws);
        std::free(io.lb_pos); std::free(io.lb_type); std::free(io.lb_time); std::free(io.lb_bpm);
        std::free(io.pr_s1); std::free(io.pr_s2); std::free(io.pr_dt);
        std::free(io.gr_id); std::free(io.gr_first); std::free(io.gr_last); std::free(io.gr_s1);
        std::free(io.gr_pairs); std::free(io.gr_dt); std::free(io.gr_bpm);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
