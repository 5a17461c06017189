/*
 * bpmx_run.h — one run of the stages (bpmx_run.hip) and the batch geometry
 * that every stage of it reads.
 */
#ifndef BPMX_RUN_H
#define BPMX_RUN_H

#include <vector>

#include "bpmx_ctx.h"

namespace bpmx {

struct RunGeo {
    int F;                             /* recordings */
    int64_t maxnd, sumnd, sumb;        /* longest decimated length, all of them, all 64-sample blocks */
    hipStream_t s;
    std::vector<int64_t> foff, doff;   /* host: [F+1] frame and decimated offsets */
    std::vector<int32_t> active;       /* host: [F] long enough to analyse */
    const int64_t *d_foff, *d_doff, *d_boff;   /* device: [F+1] frame, decimated and block-table offsets */
    const int32_t *d_active;
    int32_t *d_run1, *d_run2, *d_an1, *d_an2, *d_nraw;   /* device: [F] per-recording run masks and counts */
};

/* the stages P->stages asks for over batch B, enqueued on `stream`.
 * env_active: recordings count as active by the envelope stage's rule
 * (a pipelined chunk's detection run).  ord: bpmx_run_ordered. */
int run_impl(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O, void *stream,
             bool env_active, const bpmx_peak_order *ord = nullptr);

}  // namespace bpmx

#endif
