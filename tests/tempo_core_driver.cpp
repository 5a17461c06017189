/*
 * tempo_core_driver.cpp — runs csrc/bpmx_tempo_core.h as plain C++ for
 * tests/test_tempo_core.py and tests/test_tempo_abi.py.  Host code only.
 *
 *   tempo_core_driver IN OUT [LANES]   the cases of IN; LANES > 1: that many threads as the lanes of one
 *                                      workgroup, sync() a barrier (the kernel's partition of the work)
 *   tempo_core_driver plan [WIN:HOP:KMIN:KMAX ...]   the structure sizes, then tempo_plan of each case,
 *                                      as key=value lines
 *
 * IN:  int32 n_cases, then per case
 *        int32 nd, sr, win, hop, kmin, kmax, start_windows, 0, double min_strength, double env[nd]
 * OUT: per case
 *        int32 nw, int32 lag[nw], double rho[nw], double bpm[nw], int32 n_valid, n_strong,
 *        double median_bpm, mean_rho, hint
 *
 * The mean removal, the padding and the lag sums (steps 2 and 3) are written
 * out here in the plainest order; steps 1 and 4 to 6 and the record are the
 * core's.  Every array is its own allocation of exactly its entries (the
 * padded window of win + kmax + 1, the kmax - kmin + 3 lag sums, the outputs
 * of nw windows), so a sanitizer build reports any access beyond them.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_tempo_core.h"

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

static int plan_mode(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_out=%zu threads=%d waves=%d step=%d pad=%d lds_max=%d rec_threads=%d "
                "sizeof_best=%zu\n",
                sizeof(bpmx_tempo_params), sizeof(bpmx_tempo_out), (int)TEMPO_T, (int)TEMPO_WAVES, (int)TEMPO_U,
                (int)TEMPO_PAD, (int)TEMPO_LDS_MAX, (int)TEMPO_REC_T, sizeof(tempo_best));
    for (int i = 2; i < argc; ++i) {
        int win, hop, kmin, kmax;
        if (std::sscanf(argv[i], "%d:%d:%d:%d", &win, &hop, &kmin, &kmax) != 4) return 2;
        const TempoPlan P = tempo_plan(win, hop, kmin, kmax);
        std::printf("status=%d nlag=%d lags=%d win4=%d chunk=%d elen=%d pstride=%d lds=%zu\n", P.status, P.nlag, P.lags,
                    P.win4, P.chunk, P.elen, P.pstride, P.lds);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) return plan_mode(argc, argv);
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT [LANES] | plan [WIN:HOP:KMIN:KMAX ...]\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    const int lanes = argc > 3 ? std::atoi(argv[3]) : 1;
    if (lanes < 1 || lanes > 64) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t h[8];
        double min_strength = 0;
        if (!get(in, h, 8) || !get(in, &min_strength, 1) || h[0] < 0) return 3;
        const int32_t nd = h[0], sr = h[1], win = h[2], hop = h[3], kmin = h[4], kmax = h[5], start = h[6];
        if (tempo_plan(win, hop, kmin, kmax).status == BPMX_E_ARG) return 3;
        double *x = make<double>(nd);
        if (!get(in, x, nd)) return 3;
        const int64_t nw = tempo_windows(nd, win, hop);
        const int nlag = kmax - kmin + 3;
        int32_t *lag = make<int32_t>(nw);
        double *rho = make<double>(nw), *bpm = make<double>(nw);
        double *e = make<double>((size_t)win + kmax + 1), *r = make<double>(nlag);
        tempo_scan *scans = make<tempo_scan>(lanes);
        tempo_best *bests = make<tempo_best>(lanes);
        double r0 = 0;
        barrier bar(lanes);
        run(lanes, [&](int l) {
            const lanes_exec X{l, lanes, &bar};
            for (int64_t w = 0; w < nw; ++w) {
                const double *xs = x + w * hop;
                tempo_scan sc = tempo_scan_init();                  /* step 1 */
                for (int i = l; i < win; i += lanes) tempo_scan_add(sc, xs[i]);
                scans[l] = sc;
                X.sync();
                sc = scans[0];
                for (int k = 1; k < lanes; ++k) tempo_scan_merge(sc, scans[k]);
                X.sync();
                if (!tempo_scan_valid(sc)) {
                    if (l == 0) {
                        const tempo_val v = tempo_outputs(0, 0, 0, 0, 0, sr);
                        lag[w] = v.lag; rho[w] = v.rho; bpm[w] = v.bpm;
                    }
                    continue;
                }
                double m = 0;                                       /* steps 2 and 3 */
                for (int i = 0; i < win; ++i) m += xs[i];
                m /= (double)win;
                for (int i = l; i < win + kmax + 1; i += lanes) e[i] = i < win ? xs[i] - m : 0.0;
                X.sync();
                for (int j = l; j < nlag; j += lanes) {
                    const int k = kmin - 1 + j;
                    double s = 0;
                    for (int i = 0; i < win; ++i) s += e[i] * e[i + k];
                    r[j] = s;
                }
                if (l == 0) {
                    double s = 0;
                    for (int i = 0; i < win; ++i) s += e[i] * e[i];
                    r0 = s;
                }
                X.sync();
                const tempo_best b = tempo_pick(X, r, kmin, kmax, bests);   /* steps 4 to 6 */
                if (l == 0) {
                    const int j = b.k - (kmin - 1);
                    const tempo_val v = b.k == 0 ? tempo_outputs(0, 0, 0, 0, 0, sr)
                                                 : tempo_outputs(b.k, r[j - 1], r[j], r[j + 1], r0, sr);
                    lag[w] = v.lag; rho[w] = v.rho; bpm[w] = v.bpm;
                }
                X.sync();
            }
        });
        void *ws = std::malloc(tempo_rec_ws_bytes(lanes));
        int32_t n_valid = -1, n_strong = -1;
        double rec[3];
        tempo_rec o{&n_valid, &n_strong, &rec[0], &rec[1], &rec[2]};
        run(lanes, [&](int l) {
            tempo_record(lanes_exec{l, lanes, &bar}, nw, lag, rho, bpm, min_strength, start,
                         tempo_rec_ws_layout(ws, lanes), o);
        });
        const int32_t nw32 = (int32_t)nw;
        if (!put(out, &nw32, 1) || !put(out, lag, nw) || !put(out, rho, nw) || !put(out, bpm, nw) ||
            !put(out, &n_valid, 1) || !put(out, &n_strong, 1) || !put(out, rec, 3))
            return 5;
        std::free(x); std::free(lag); std::free(rho); std::free(bpm); std::free(e); std::free(r);
        std::free(scans); std::free(bests); std::free(ws);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
