/*
 * hrvspec_core_driver.cpp — runs csrc/bpmx_hrvspec_core.h as plain C++ for
 * tests/test_hrvspec_core.py and tests/test_hrvspec_abi.py.  Host code only.
 *
 *   hrvspec_core_driver IN OUT [LANES] [direct]   the cases of IN; LANES > 1: that many threads as the lanes
 *                                      of one workgroup, sync() a barrier; direct: one sincos per term
 *                                      instead of the rotation along the grid
 *   hrvspec_core_driver plan [WIN:DMIN ...]   the structure sizes, then hrvspec_plan of each case (the other
 *                                      parameters valid), as key=value lines
 *
 * IN:  int32 n_cases, then per case
 *        int32 n_final, sr, beats status, 0, int64 nd, bpmx_hrvspec_params, int32 final_idx[n_final]
 * OUT: per case
 *        int32 status, nw, int32 code[nw], n_rr[nw], lf_peak[nw], hf_peak[nw],
 *        double t_mid[nw], var[nw], lf[nw], hf[nw], q[nw][n_freq], record[8]
 *
 * A lane takes every LANES-th block of 8 frequencies (or every LANES-th
 * frequency) over all the intervals: the kernel's own partition is another,
 * the arithmetic is the core's.  Every array is its own allocation of exactly
 * its entries (the four interval arrays of nmax, q of n_freq, the outputs of
 * nw windows), so a sanitizer build reports any access beyond them.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../bpm_analysis_amd/csrc/bpmx_hrvspec_core.h"

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
    int count(int flag, int32_t *ws, int *total) const {
        ws[l] = flag;
        sync();
        int before = 0, all = 0;
        for (int k = 0; k < w; ++k) {
            before += k < l ? ws[k] : 0;
            all += ws[k];
        }
        sync();
        *total = all;
        return before;
    }
};

template <class F>
static void run(int lanes, F body) {
    std::vector<std::thread> pool;
    for (int l = 1; l < lanes; ++l) pool.emplace_back(body, l);
    body(0);
    for (auto &t : pool) t.join();
}

static bpmx_hrvspec_params valid_params() {
    bpmx_hrvspec_params P{};
    P.win = 36240; P.hop = 9060; P.dmin = 76; P.dmax = 453; P.min_intervals = 16; P.min_span = 7550;
    P.n_freq = 256; P.lf_a = 0; P.lf_b = 78; P.hf_a = 78; P.hf_b = 256;
    P.om0 = 8.3e-4; P.dom = 2.9e-5; P.scale = 4.7e-6;
    return P;
}

static int plan_mode(int argc, char **argv) {
    std::printf("sizeof_params=%zu sizeof_out=%zu threads=%d block=%d parts=%d max_freq=%d per=%d lds_max=%d "
                "rec_threads=%d sizeof_pick=%zu record=%d\n",
                sizeof(bpmx_hrvspec_params), sizeof(bpmx_hrvspec_out), (int)HRVSPEC_T, (int)HRVSPEC_B,
                (int)HRVSPEC_PARTS, (int)HRVSPEC_MAX_FREQ, (int)HRVSPEC_PER, (int)HRVSPEC_LDS_MAX, (int)HRVSPEC_REC_T,
                sizeof(hrvspec_pick), (int)BPMX_HRVSPEC_RECORD);
    for (int i = 2; i < argc; ++i) {
        bpmx_hrvspec_params P = valid_params();
        if (std::sscanf(argv[i], "%d:%d", &P.win, &P.dmin) != 2) return 2;
        if (P.dmax < P.dmin) P.dmax = P.dmin;
        const HrvspecPlan G = hrvspec_plan(P);
        std::printf("status=%d nmax=%d lds=%zu\n", G.status, G.nmax, G.lds);
    }
    return 0;
}

template <int B, bool ROT>
static void spectrum(const lanes_exec &X, const hrvspec_ws &w, const hrvspec_head &H, const bpmx_hrvspec_params &P,
                     double *q) {
    const int nblk = (P.n_freq + B - 1) / B;
    for (int blk = X.lane(); blk < nblk; blk += X.width()) {
        double acc[HS_NSUM][B];
        for (int i = 0; i < HS_NSUM; ++i)
            for (int k = 0; k < B; ++k) acc[i][k] = 0.0;
        hrvspec_accum<B, ROT>(w, H.n, 0, 1, blk * B, P, acc);
        for (int k = 0; k < B && blk * B + k < P.n_freq; ++k) {
            double sum[HS_NSUM];
            for (int i = 0; i < HS_NSUM; ++i) sum[i] = acc[i][k];
            q[blk * B + k] = hrvspec_power(sum, H.n, H.Y, H.YY);
        }
    }
    X.sync();
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) return plan_mode(argc, argv);
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN OUT [LANES] [direct] | plan [WIN:DMIN ...]\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    const int lanes = argc > 3 ? std::atoi(argv[3]) : 1;
    const bool rot = !(argc > 4 && std::strcmp(argv[4], "direct") == 0);
    if (lanes < 1 || lanes > 64) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t h[4];
        int64_t nd = 0;
        bpmx_hrvspec_params P;
        if (!get(in, h, 4) || !get(in, &nd, 1) || !get(in, &P, 1) || h[0] < 0) return 3;
        const int32_t n_final = h[0], sr = h[1], bst = h[2];
        const HrvspecPlan G = hrvspec_plan(P);
        if (G.status != BPMX_OK) return 3;
        int32_t *idx = make<int32_t>(n_final);
        if (!get(in, idx, n_final)) return 3;
        const int64_t nw = hrvspec_windows(nd, P.win, P.hop);
        const bool none = bst != 0 || n_final < 2;
        int32_t *code = make<int32_t>(nw), *n_rr = make<int32_t>(nw), *lfp = make<int32_t>(nw), *hfp = make<int32_t>(nw);
        double *t_mid = make<double>(nw), *var = make<double>(nw), *lf = make<double>(nw), *hf = make<double>(nw);
        double *qq = make<double>((size_t)nw * P.n_freq), *q = make<double>(P.n_freq);
        hrvspec_ws w;
        w.s = make<double>(G.nmax); w.u = make<double>(G.nmax); w.cd = make<double>(G.nmax); w.sd = make<double>(G.nmax);
        w.dw = make<double>(lanes); w.iw = make<int32_t>(lanes); w.pk = make<hrvspec_pick>(lanes);
        barrier bar(lanes);
        run(lanes, [&](int l) {
            const lanes_exec X{l, lanes, &bar};
            for (int64_t b = 0; b < nw; ++b) {
                const hrvspec_head H = hrvspec_stage(X, idx, none ? 0 : n_final, b * (int64_t)P.hop, P, sr, G.nmax, rot, w);
                double *row = qq + b * (int64_t)P.n_freq;
                if (H.code != 0) {
                    if (l == 0) {
                        code[b] = H.code; n_rr[b] = H.n; lfp[b] = hfp[b] = -1;
                        t_mid[b] = H.t_mid; var[b] = lf[b] = hf[b] = hs_nan();
                        for (int m = 0; m < P.n_freq; ++m) row[m] = hs_nan();
                    }
                    X.sync();
                    continue;
                }
                if (rot) spectrum<HRVSPEC_B, true>(X, w, H, P, q); else spectrum<1, false>(X, w, H, P, q);
                const hrvspec_bandval a = hrvspec_band(X, q, P.lf_a, P.lf_b, w);
                const hrvspec_bandval d = hrvspec_band(X, q, P.hf_a, P.hf_b, w);
                if (l == 0) {
                    const double k = P.scale * (H.e_last - H.e_first) * H.var;
                    code[b] = 0; n_rr[b] = H.n; lfp[b] = a.peak; hfp[b] = d.peak;
                    t_mid[b] = H.t_mid; var[b] = H.var;
                    lf[b] = P.lf_b > P.lf_a ? k * a.sum : 0.0;
                    hf[b] = P.hf_b > P.hf_a ? k * d.sum : 0.0;
                    std::memcpy(row, q, sizeof(double) * P.n_freq);
                }
                X.sync();
            }
        });
        double rec[BPMX_HRVSPEC_RECORD];
        double *st = make<double>(3 * (size_t)lanes);
        run(lanes, [&](int l) { hrvspec_record(lanes_exec{l, lanes, &bar}, nw, code, lf, hf, st, rec); });
        const int32_t head[2] = {none ? BPMX_HRVSPEC_NONE : BPMX_HRVSPEC_OK, (int32_t)nw};
        if (!put(out, head, 2) || !put(out, code, nw) || !put(out, n_rr, nw) || !put(out, lfp, nw) || !put(out, hfp, nw) ||
            !put(out, t_mid, nw) || !put(out, var, nw) || !put(out, lf, nw) || !put(out, hf, nw) ||
            !put(out, qq, (size_t)nw * P.n_freq) || !put(out, rec, BPMX_HRVSPEC_RECORD))
            return 5;
        std::free(idx); std::free(code); std::free(n_rr); std::free(lfp); std::free(hfp); std::free(t_mid);
        std::free(var); std::free(lf); std::free(hf); std::free(qq); std::free(q); std::free(w.s); std::free(w.u);
        std::free(w.cd); std::free(w.sd); std::free(w.dw); std::free(w.iw); std::free(w.pk); std::free(st);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
