// amc_commit_dev.h — the commit of a resolved p-p sweep: completed paths -> histograms / records, collision counters,
// overlay lists emptied, and (unless the results stay in the slot arrays for the next streaming pass) scratch state ->
// particle arrays.  It is wide, order-free work on a few hundred to a few ten thousand entries, and nothing between a
// sweep and the next streaming pass depends on it — so inside a run it RIDES ALONG with that pass (the first blocks of
// k_stream do it, amc_stream.hip) instead of costing a launch of its own; k_commit (amc_resolve.hip) is the stand-alone
// form for a sweep that is followed by something else (a read-back, a stage call).
#pragma once
#include "amc_grid_dev.h"

#define AMC_COMMIT_BLOCKS 64        // blocks of 256 threads that share the commit

struct amc_commit_args {
    amc_resolve_ctl *ctl;           // what the ordered workgroup left: counts, ok flag
    const double4 *hist;
    int *ov_head;
    const int *ev_gen;
    const rs_event *ev;
    const int4 *sl_meta;
    const int *sl_hits;
    const uint8_t *sl_moved;
    const double *sl_state;
    int *slot_of;
    int max_slots, max_hist;
    long long lo, hi;               // owned particle range: a completed path is emitted by the owner of its particle
    int count_pp;                   // this rank adds the sweep's collision count (multi-GPU: the rank that owns particle 0)
    int defer;                      // results stay in the slot arrays (the streaming pass picks them up through slot_of[])
    int nogrid;
    int enabled;
    int step;                       // the `step` key of the paths this commit emits: the index of the sweep's own step
    // the ordered workgroup on demand (amc_internal.h).  od_stall: the sticky word — the commit (and the pass it rides along
    // with) of a step later than it does nothing.  from_wide: no ordered pass ran for this sweep, so nobody has handed its
    // counts over: they are taken from the wide kernel's own words, and this commit does what the idle ordered workgroup
    // did besides — the candidate counter cleared, the candidate count told to the host.  (The wide kernel's words are
    // re-armed by the next detect kernel: every block here reads them.)
    const int *od_stall;
    int od_tick;
    int from_wide;
    const int *wctl;
    int *host_ncand;
};

AMC_DEV void amc_commit_part(const amc_commit_args &C, const amc_out &O, const amc_grid &G, const amc_state &S, int gtid,
                             int gstride)
{
    amc_resolve_ctl *ctl = C.ctl;
    int c_active, c_ok, c_nslots, c_nhist, c_ncand, c_nclusters = 0, c_rounds;
    if (C.from_wide) {
        // (candidate k owns slots 2k, 2k + 1 and the history pairs 4k, 4k + 2; what the wide kernel took from its counters
        // comes after those — the sums the idle ordered workgroup handed over)
        const amc_resolve_ctl *wc = (const amc_resolve_ctl *)C.wctl;
        c_ncand = wc->ncand;
        c_active = c_ncand > 0;
        c_nslots = 2 * c_ncand + wc->nslots; c_nhist = 4 * c_ncand + wc->nhist;
        c_ok = !wc->ovf; c_rounds = 1;
        if (gtid == 0) {
            for (int b = 0; b < 16; b++) c_nclusters += C.wctl[32 + b];
            if (C.host_ncand) *C.host_ncand = c_ncand;
            O.cnt->cand_count = 0;
        }
    } else {
        c_active = ctl->active; c_ok = ctl->ok && !ctl->ovf; c_nslots = ctl->nslots; c_nhist = ctl->nhist;
        c_ncand = ctl->ncand; c_rounds = ctl->rounds;
        if (gtid == 0) c_nclusters = ctl->nclusters;
    }
    if (!c_active) return;
    const bool ok = c_ok != 0;
    const bool defer = ok && C.defer;
    const int ns = c_nslots < C.max_slots ? c_nslots : C.max_slots;
    const int nh = c_nhist < C.max_hist ? c_nhist : C.max_hist;
    int my_hits = 0, my_fp = 0;
    for (int s = gtid; s < ns; s += gstride) {
        const int p = C.sl_meta[s].x;
        if (ok && C.count_pp) { const int hs = C.sl_hits[s]; my_hits += hs & 0xffff; my_fp += hs >> 16; }
        if (defer || p < 0) continue;               // (a candidate's slot that no particle took has p = -1)
        if (ok && C.sl_moved[s]) {
            const double *t = C.sl_state + (size_t)s * RS_SLOT_DOUBLES;
            S.x[p] = t[0]; S.y[p] = t[1]; S.z[p] = t[2]; S.vx[p] = t[3]; S.vy[p] = t[4]; S.vz[p] = t[5];
            S.d[p] = t[6]; S.dx[p] = t[7]; S.dy[p] = t[8]; S.dz[p] = t[9]; S.flag[p] = t[10] != 0.0 ? 1 : 0;
        }
        C.slot_of[p] = -1;
    }
    // one atomic per wave instead of one per slot on a single counter word
    for (int o = 32; o > 0; o >>= 1) { my_hits += __shfl_down(my_hits, o, 64); my_fp += __shfl_down(my_fp, o, 64); }
    if ((threadIdx.x & 63) == 0 && my_hits) atomicAdd(&O.banks[amc_bank_id()].n_pp, (unsigned long long)my_hits);
    if ((threadIdx.x & 63) == 0 && my_fp) atomicAdd(&O.banks[amc_bank_id()].n_fp_errors, (unsigned long long)my_fp);
    if (ok)
        for (int e = gtid; e < nh; e += gstride) {
            const int g = C.ev_gen[e];
            if (g == 0) continue;                                       // no completed path at this entry
            const rs_event ev = C.ev[e];
            if (g != C.sl_meta[ev.slot].z) continue;                    // event of an emulation that was redone since
            const int owner = ev.which ? ev.i : ev.j;                   // the particle whose free path completed
            if (owner < C.lo || owner >= C.hi) continue;
            amc_emit(O, ev.phase, ev.cell, ev.i, ev.j, ev.which, ev.val[0], ev.val[1], ev.val[2], ev.val[3]);
        }
    if (!C.nogrid)
        for (int h = gtid; h < nh; h += gstride) {                      // overlay entries of this sweep
            const double4 r = C.hist[h];
            int cx, cy, cz;
            amc_grid_coords(G, r.x, r.y, r.z, cx, cy, cz);
            C.ov_head[amc_grid_cell(G, cx, cy, cz, nullptr)] = -1;
        }
    if (gtid == 0) {
        amc_dev_counters *cnt = O.cnt;
        cnt->n_candidates += (unsigned long long)c_ncand;
        cnt->n_clusters += (unsigned long long)c_nclusters;
        cnt->n_rounds += (unsigned long long)c_rounds;
        if (!ok) cnt->flags |= 4ULL;
        ctl->lazy_ns = defer ? ns : 0;
    }
}
