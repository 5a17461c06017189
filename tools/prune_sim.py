"""Simulate the value-bin pruning of the final-floor rolling quantile on
synthetic recordings: fraction of the curve's samples that can ever be a
window's k-th or (k+1)-th smallest (exact bound, 64 value bins, 64-output
blocks).  Prints the upper bound alone (b*) and both sides (b* and a*, the
bin of the k_min-th smallest of a block's windows' union: samples below it
are only counted).  Host-only study tool."""
import sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O
from bpm_analysis_amd.config import DEFAULT_PARAMS

NB = int(sys.argv[2]) if len(sys.argv) > 2 else 64


def keep_fraction(dense, t0, W, q, nbins=NB, blk=64):
    n = dense.size
    v = dense[t0:]
    vmin, vmax = v.min(), v.max()
    scale = (nbins - 1e-9) / (vmax - vmin) if vmax > vmin else 0.0
    bins = np.full(n, -1)
    bins[t0:] = np.minimum(((v - vmin) * scale).astype(np.int64), nbins - 1)
    off = (W - 1) // 2
    nbk = (n + blk - 1) // blk
    bstar = np.full(nbk, nbins - 1)
    astar = np.zeros(nbk, np.int64)
    for B in range(nbk):
        i0, i1 = B * blk, min(n, B * blk + blk) - 1
        e0 = min(i0 + 1 + off, n); s1 = max(min(i1 + 1 + off, n) - W, 0)
        s0 = max(e0 - W, 0); e1 = min(i1 + 1 + off, n)
        lo, hi = max(s1, t0), e0            # intersection of the block's windows
        kq = []
        for i in (i0, i1):
            e = min(i + 1 + off, n); s = max(e - W, 0); nobs = e - max(s, t0)
            kq.append(int(q * (nobs - 1)) if nobs > 1 else 0)
        kmax, kmin = max(kq), min(kq)
        if hi - lo >= kmax + 2:
            c = np.cumsum(np.bincount(bins[lo:hi], minlength=nbins))
            bstar[B] = int(np.searchsorted(c, kmax + 2))
        ulo, uhi = max(s0, t0), e1          # union of the block's windows
        if uhi > ulo:
            cu = np.cumsum(np.bincount(bins[ulo:uhi], minlength=nbins))
            if cu[-1] >= kmin + 1:
                astar[B] = int(np.searchsorted(cu, kmin + 1))
    # thresholds per position: over the blocks whose union window contains it
    thr = np.full(n, -1)
    lthr = np.full(n, nbins)
    for B in range(nbk):
        i0, i1 = B * blk, min(n, B * blk + blk) - 1
        s0 = max(min(i0 + 1 + off, n) - W, 0); e1 = min(i1 + 1 + off, n)
        thr[s0:e1] = np.maximum(thr[s0:e1], bstar[B])
        lthr[s0:e1] = np.minimum(lthr[s0:e1], astar[B])
    b = bins[t0:]
    upper = b <= thr[t0:]
    return upper.mean(), (upper & (b >= lthr[t0:])).mean()


def half_kept(dense, tr, W, q, c, nbins=64, blk=64):
    """Kept samples of half c of k_floor_wm_half, following the kernel's own
    arithmetic: outputs [c h, min(n, (c + 1) h)), the samples [t0, top) their
    windows reach, bins over the staged troughs' value range, b* from full
    position blocks of the common window, a* from the blocks covering the
    union.  Returns (kept, samples in reach)."""
    n = dense.size
    off = (W - 1) // 2
    h = ((n + 1) // 2 + 63) // 64 * 64
    o0, o1 = c * h, min(n, (c + 1) * h)

    def win(i):
        e = min(i + 1 + off, n)
        return max(i + 1 + off - W, 0), e

    t0 = max(win(o0)[0], int(tr[0]))
    top = win(o1 - 1)[1]
    if top <= t0:
        return 0, 0
    jlo = max(int(np.searchsorted(tr, t0, side="right")) - 1, 0)
    jhi = min(int(np.searchsorted(tr, top - 1, side="left")), tr.size - 1)
    tv = dense[tr[jlo:jhi + 1]]
    vmin, span = tv.min(), tv.max() - tv.min()
    scale = nbins / span if span > 0 else 0.0
    tt = (dense[t0:top] - vmin) * scale
    bins = np.where(tt > 0, np.minimum(tt, nbins - 1), 0).astype(np.int64)
    mall = top - t0
    npb = (mall + 63) // 64
    cum = np.zeros((npb + 1, nbins), np.int64)              # samples of blocks < r with bin <= b
    for r in range(npb):
        cum[r + 1] = cum[r] + np.cumsum(np.bincount(bins[r * 64:r * 64 + 64], minlength=nbins))
    nbo = (o1 - o0 + 63) // 64
    bstar = np.full(nbo, nbins - 1)
    astar = np.zeros(nbo, np.int64)
    for B in range(nbo):
        ib = o0 + B * blk
        ie = min(o1, ib + blk) - 1
        (s0, e0), (s1, e1) = win(ib), win(ie)
        nb = min(W, e1 - max(s0, t0))
        kq = int(q * (nb - 1)) if nb > 1 else 0
        clo, chi = max(s1, t0) - t0, e0 - t0
        pbs, pbe = (clo + 63) // 64, max(chi, 0) // 64
        if pbe > pbs and cum[pbe, -1] - cum[pbs, -1] >= kq + 2:
            bstar[B] = int(np.searchsorted(cum[pbe] - cum[pbs], kq + 2))
        nmin = min(e0 - max(s0, t0), e1 - max(s1, t0))
        kmin = int(q * (nmin - 1)) if nmin > 1 else 0
        ulo, uhi = max(s0, t0) - t0, e1 - t0
        cbs, cbe = max(ulo, 0) // 64, (min(npb, (uhi + 63) // 64) if uhi > 0 else 0)
        if cbe > cbs and nmin > 0 and cum[cbe, -1] - cum[cbs, -1] >= kmin + 1:
            astar[B] = int(np.searchsorted(cum[cbe] - cum[cbs], kmin + 1))
    kept = 0
    for pb in range(npb):
        a = t0 + pb * 64
        ilo, ihi = max(a - off, 0), min(n - 1, a + 63 + W - off)
        if ihi >= n - 1 - off:
            ihi = n - 1
        ilo, ihi = max(ilo, o0), min(ihi, o1 - 1)
        if ihi < ilo:
            continue
        B0, B1 = (ilo - o0) // 64, (ihi - o0) // 64
        thr, lthr = bstar[B0:B1 + 1].max(), astar[B0:B1 + 1].min()
        b = bins[pb * 64:pb * 64 + 64]
        kept += int(((b >= lthr) & (b <= thr)).sum())
    return kept, mall


def halves_of_seed(seed):
    p = dict(DEFAULT_PARAMS)
    pcm = O.synth(seed, 2646000, 44100)
    d = O.derive(44100, p)
    env = O.preprocess_native(pcm, d)
    floor, tr, flags = O.noise_floor(env, d, p)
    if tr.size <= 2:
        return seed, None
    dense = O.interp_dense(tr, env)
    return seed, [half_kept(dense, tr, d.noise_window, p["noise_floor_quantile"], c) for c in (0, 1)]


if len(sys.argv) > 1 and sys.argv[1] == "halves":
    # python tools/prune_sim.py halves [seeds] [processes]: the kept samples of
    # each half of the bench recordings against k_floor_wm_half's cap
    from multiprocessing import Pool
    nseed = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    with Pool(int(sys.argv[3]) if len(sys.argv) > 3 else 8) as pool:
        rows = [r for _, r in pool.imap_unordered(halves_of_seed, range(nseed), chunksize=8) if r]
    k = np.array([[a[0], b[0]] for a, b in rows])
    r = np.array([[a[1], b[1]] for a, b in rows])
    for c in (0, 1):
        print("half %d over %d seeds: kept min %d p50 %d p99 %d max %d; in reach max %d" % (
            c, len(rows), k[:, c].min(), np.median(k[:, c]), np.percentile(k[:, c], 99), k[:, c].max(), r[:, c].max()))
    print("cap 4224: headroom over the largest half %.0f %%" % (100.0 * (4224 / k.max() - 1)))
    sys.exit(0)

p = dict(DEFAULT_PARAMS)
fr = []
for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 6):
    pcm = O.synth(seed, 2646000, 44100)
    d = O.derive(44100, p)
    env = O.preprocess_native(pcm, d)
    floor, tr, flags = O.noise_floor(env, d, p)
    dense = O.interp_dense(tr, env)
    fr.append(keep_fraction(dense, int(tr[0]), d.noise_window, p["noise_floor_quantile"]))
    print(seed, len(tr), "upper bound %.3f, both sides %.3f" % fr[-1])
print("mean keep (upper, both sides)", np.mean(fr, axis=0))
