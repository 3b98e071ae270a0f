// The EM fits of the C ABI (include/wgsassign_hip.h: wgs_em_*): emMAF.py:15-27 as ONE call per batch of fits (wgs_em_fit: iterations
// enqueued ahead of the host, decisions on the device), the step-by-step twin, the exact convergence chain, and the policy that decides
// which sweep kernel a batch takes (direct, grouped leave-one-out, class-coded -- and when the codes are worth building).
// Host-side orchestration only; the arithmetic is in em_kernels.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "common.h"
#include "em_state.h"
#include "stream_checks.h"
#include "streams.h"
#include "zscore.h"

// Enqueues `units` fits or fit groups as launch(first, count) over slices of at most `per_launch` of them.
template <class Launch> static int em_launch_sliced(size_t units, size_t per_launch, Launch launch)
{
    for (size_t off = 0; off < units; off += per_launch)
        if (launch(off, (int)std::min(per_launch, units - off))) return 1;
    return 0;
}

extern "C" {

/* ------------------------------------------------------------------ EM */

// (struct wgs_em: em_state.h)

void wgs_em_destroy(wgs_em *em)
{
    if (!em || !wgs_live_remove(em)) return;          // (destroyed already, e.g. together with its matrix)
    (void)hipSetDevice(em->b->ctx->device);
    for (int i = 0; i < 3; ++i)
        if (em->fbuf[i]) (void)hipFree(em->fbuf[i]);
    if (em->d_part_b) (void)hipFree(em->d_part_b);
    if (em->d_ssq) (void)hipFree(em->d_ssq);
    if (em->d_part) (void)hipFree(em->d_part);
    if (em->d_part2) (void)hipFree(em->d_part2);
    if (em->d_carry) (void)hipFree(em->d_carry);
    if (em->d_chain_work) (void)hipFree(em->d_chain_work);
    if (em->ev0) (void)hipEventDestroy(em->ev0);
    if (em->ev1) (void)hipEventDestroy(em->ev1);
    for (hipEvent_t e : em->ev_sw) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (em->d_descs[i]) (void)hipFree(em->d_descs[i]);
        if (em->h_descs[i]) (void)hipHostFree(em->h_descs[i]);
        if (em->d_groups[i]) (void)hipFree(em->d_groups[i]);
        if (em->h_groups[i]) (void)hipHostFree(em->h_groups[i]);
        if (em->h_state[i]) (void)hipHostFree(em->h_state[i]);
        if (em->h_ssq[i]) (void)hipHostFree(em->h_ssq[i]);
        if (em->ev_it[i]) (void)hipEventDestroy(em->ev_it[i]);
    }
    for (void *p : {(void *)em->d_state, (void *)em->d_ssq2, (void *)em->d_jobs, (void *)em->d_chain_out, em->d_chain_batch})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)em->h_jobs, (void *)em->h_chain_out, (void *)em->h_setstate})
        if (p) (void)hipHostFree(p);
    delete em;
}

int wgs_em_create(wgs_beagle *b, int32_t n_fits, const int32_t *fit_group, const int32_t *fit_skip, int mode, wgs_em **out)
{
    WGS_REQUIRE(b && fit_group && out, "null argument");
    WGS_REQUIRE(n_fits > 0, "n_fits must be positive");
    WGS_REQUIRE(mode == WGS_MODE_EXACT || mode == WGS_MODE_FAST, "unknown mode %d", mode);
    HIP_TRY(hipSetDevice(b->ctx->device));
    wgs_em *em = new wgs_em();
    wgs_live_add(em, WGS_LIVE_EM, b);
    auto guard = on_failure([&] { wgs_em_destroy(em); });
    em->b = b;
    em->n_fits = n_fits;
    em->cap_m = b->m;
    em->mode = mode;
    em->group.resize(n_fits);
    em->skip_local.resize(n_fits);
    em->n_eff.resize(n_fits);
    em->cur.assign(n_fits, 0);
    em->prev.assign(n_fits, 1);
    em->fuse_used.assign(n_fits, 1);
    em->pend_cur.assign(n_fits, 0);
    em->pend_prev.assign(n_fits, 1);
    em->active.assign(n_fits, 1);
    for (int j = 0; j < n_fits; ++j) {
        const int g = fit_group[j];
        if (g < 0 || g >= b->n_groups || b->slabs[g].ncols == 0) {
            wgs_set_error("fit %d: group %d is out of range or empty", j, g);
            return 2;
        }
        int skip = -1;
        if (fit_skip && fit_skip[j] >= 0) {
            const int i = fit_skip[j];
            if (i >= b->n || b->group_of[i] != g) {
                wgs_set_error("fit %d: left-out individual %d does not belong to group %d", j, i, g);
                return 2;
            }
            skip = b->col_of[i];
        }
        em->group[j] = g;
        em->skip_local[j] = skip;
        em->n_eff[j] = b->slabs[g].ncols - (skip >= 0 ? 1 : 0);
    }
    const size_t fbytes = (size_t)n_fits * b->m * sizeof(float);
    for (int i = 0; i < 2; ++i) {
        if (wgs_malloc(&em->fbuf[i], fbytes) != hipSuccess) {
            wgs_set_error("hipMalloc of %zu bytes for EM frequencies failed", fbytes);
            return 1;
        }
    }
    HIP_TRY(wgs_malloc(&em->d_ssq, sizeof(double) * n_fits));
    HIP_TRY(wgs_malloc(&em->d_part, sizeof(double) * (size_t)n_fits * wgs_ntiles(b->m)));
    HIP_TRY(wgs_malloc(&em->d_part2, sizeof(double) * (size_t)n_fits * ssq_reduce_chunks()));
    HIP_TRY(wgs_malloc(&em->d_carry, 2 * sizeof(float)));
    HIP_TRY(wgs_malloc(&em->d_chain_work, rmse_chain_workspace_bytes(b->m)));
    HIP_TRY(hipEventCreate(&em->ev0));
    HIP_TRY(hipEventCreate(&em->ev1));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(wgs_malloc(&em->d_descs[i], sizeof(FitDesc) * n_fits));
        HIP_TRY(hipHostMalloc(&em->h_descs[i], sizeof(FitDesc) * n_fits, hipHostMallocDefault));
        HIP_TRY(wgs_malloc(&em->d_groups[i], sizeof(int32_t) * 2 * n_fits));
        HIP_TRY(hipHostMalloc(&em->h_groups[i], sizeof(int32_t) * 2 * n_fits, hipHostMallocDefault));
    }
    if (launch_fill(b->ctx, em->fbuf[0], (int64_t)n_fits * b->m, 0.25f)) return 1;   // emMAF.py:17-18
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    guard.dismiss();
    *out = em;
    return 0;
}


/* Whether building the class codes pays for the EM sweeps still to come (codes.hip builds them in one pass over the matrix):
 *   the encode pass costs wgs_codes_build_ms_estimate (the matrix's bytes at ~1.8 TB/s, more with larger hash tables);
 *   a coded sweep saves a share of the direct sweep (the slabs' bytes at ~6 TB/s) that depends on how many of a population's
 *   individuals share a class: min(0.6, 1.0 - 2.2 x classes / individuals) (em_codes_model has the measurements; round 4's
 *   0.92 - 2.72 x was fitted before a coded sweep ran two iterations);
 *   sweeps to come: what the caller knows -- wgs_em_fit its iteration limit, of which a fit rarely uses more than ~14 (the
 *   reference's default tolerance: 11-17 iterations on every data set here); a step-by-step caller nothing, so there a matrix
 *   that has been swept directly three times is taken to be in a long run.
 * A first estimate assumes fixed-error low-depth data (no sample pass: small matrices are turned away for free); when that says yes
 * the sample pass (~0.4 ms, once per matrix) supplies the matrix's own classes per slab and table size.
 * WGSASSIGN_EM_CODES_SWEEPS=k replaces the model by "k or more sweeps ahead" (0: always; tests). */
// Share of a leave-one-out sweep's time the codes save (<= 0: none).  Such batches (many fits per slab) are bound by instruction
// issue, not by memory: em_sweep_group_kernel spends 25.9 vector instructions per (fit, SNP, individual) term; through the codes
// (em_coded_group_kernel) a (fit, SNP) costs one quotient (29 instructions) per table row of its tile -- the richest SNP of the
// tile, ~1.7 x the mean classes per (slab, SNP) -- 4 per individual, and the equivalent of ~250 more in issue slots it leaves open
// (measured at 2M x 500, K=8, 62 individuals per slab and 12.7 classes: 458 ms of sweeps against 655).
static double loo_codes_saving(const wgs_codes_plan *P, double cols)
{
    if (!P || P->state <= 0 || P->lrows == 0) return 0.0;
    return 1.0 - (1.7 * P->mean_l * 29.0 + 4.0 * cols + 250.0) / (25.9 * std::max(1.0, cols));
}

// The model's own numbers for a batch of fits that sweep `swept` bytes of slabs with `cols` individuals per slab on average: what a
// sweep over the float32 slabs takes, the share of it a coded sweep saves, what the encode pass costs.  em_codes_decide decides with
// them for em_codes_pay and for wgs_codes_model, which hands them out, so that what is reported beside a measurement is what decided.
struct EmCodesModel {
    double direct_ms = 0.0, saves = 0.0, build_ms = 0.0;
    bool sampled = false;          // saves / build_ms come from the matrix's own sample pass (else from the fixed-error typical)
    bool codable = false;          // the sample pass found the matrix worth coding, with the slabs' own numbering
    bool pays = false;             // em_codes_decide: the sweeps ahead repay the encode pass
};
static EmCodesModel em_codes_model(wgs_beagle *b, double swept, double cols, bool shared, bool sample)
{
    EmCodesModel M;
    if (shared) {
        constexpr double LOO_MS_PER_TERM = 7.6e-10;          // em_sweep_group_kernel, per (fit, SNP, individual)
        M.direct_ms = swept / 8.0 * LOO_MS_PER_TERM;
    } else {
        M.direct_ms = swept / 6.0e9;
        // fixed-error 2x data shows ~4.6 * cols^0.25 classes per (slab, SNP): 14.7 at 100, 12.7 at 62, 10.5 at 40
        M.saves = wgs_em_codes_saving(4.6 * pow(std::max(1.0, cols), 0.25), cols, 24);
        M.build_ms = wgs_codes_build_ms_estimate(b, 64);
        M.codable = true;
        if (!sample) return M;
    }
    const wgs_codes_plan *P = wgs_beagle_codes_plan(b);
    M.sampled = true;
    M.codable = P && P->state > 0 && P->lrows > 0;
    if (!M.codable) {
        M.saves = 0.0;
        return M;
    }
    M.saves = shared ? std::max(0.0, loo_codes_saving(P, cols)) : wgs_em_codes_saving(P->mean_l, cols, P->lrows);
    M.build_ms = wgs_codes_build_ms_estimate(b, P->slots);
    return M;
}

// Whether the codes pay for a batch of fits with `ahead` sweeps to come, and the model that said so: a first estimate with the
// classes typical of fixed-error data turns small matrices away without a sample pass, else the matrix's own sample pass decides.
static EmCodesModel em_codes_decide(wgs_beagle *b, double swept, double cols, bool shared, double ahead)
{
    const EmCodesModel T = em_codes_model(b, swept, cols, false, false);
    if (!shared && ahead * T.saves * T.direct_ms <= T.build_ms) return T;
    EmCodesModel M = em_codes_model(b, swept, cols, shared, true);
    M.pays = M.codable && ahead * M.saves * M.direct_ms > M.build_ms;
    return M;
}

static int env_int(const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; }

// The environment switches of the sweeps' policy, read where wgs_em_step_dev / wgs_em_fit construct it (tests change them between calls)
struct EmSwitches {
    bool codes = !codes_switched_off();                         // WGSASSIGN_CODES=0: no codes at all -- and no sample pass to decide about them
    bool loo_codes = env_int("WGSASSIGN_LOO_CODES", 1) != 0;    // 0: leave-one-out batches keep the float32 kernel
    int codes_min = env_int("WGSASSIGN_EM_CODES_MIN", 28);      // smallest population swept through the codes (tests lower it)
    bool sweeps_set = getenv("WGSASSIGN_EM_CODES_SWEEPS") != nullptr;    // =k: "k or more sweeps ahead" replaces the cost models
    int sweeps_min = env_int("WGSASSIGN_EM_CODES_SWEEPS", 0);   //   (0: always; tests)
    bool fuse = env_int("WGSASSIGN_EM_FUSE", 2) >= 2;           // 0 or 1: one iteration per sweep
};

static bool em_codes_pay(const wgs_em *em, double swept, double cols, int sweeps_ahead, bool shared, const EmSwitches &sw)
{
    wgs_beagle *b = em->b;
    if (sw.sweeps_set) return sweeps_ahead >= sw.sweeps_min || b->direct_sweeps >= 3;
    // a fit uses ~14 iterations: what this one has done already (the codes' memory may arrive in the middle of it) no longer counts --
    // but a fit that has gone past 14 is taken to need a few more
    double ahead = std::min<double>(sweeps_ahead, std::max(3, 14 - em->fit_iterations));
    if (sweeps_ahead <= 0 && b->direct_sweeps >= 3) ahead = 12;
    return em_codes_decide(b, swept, cols, shared, ahead).pays;
}

/* The cost models' own predictions for this matrix (so that a caller can print them beside what it measures: bench.py,
 * tests/test_gpu_codes.py): the fits of --get_reference_af (one per population slab) and a --get_pop_like sweep over K populations.
 * out[0..11]: EM sweep over the float32 slabs, ms | share of it a coded sweep saves | encode pass incl. the slabs' numbering, ms |
 * sweeps the decision counts (14) | 1 = the model builds the codes for such a fit | scoring sweep over the float32 slabs, ms | share
 * of it the coded sweep costs | encode pass for scoring alone, ms | 1 = the model builds them for scoring | 1 = predictions from the
 * matrix's own sample pass | classes per (slab, SNP) in the sample | classes per SNP in the sample.  Runs the sample pass (~0.4 ms)
 * unless the first estimate already turns the matrix away. */
int wgs_codes_model(wgs_beagle *b, int32_t K_score, double *out)
{
    WGS_REQUIRE(b && out, "null argument");
    HIP_TRY(hipSetDevice(b->ctx->device));
    double swept = 0.0, cols = 0.0;
    int groups = 0;
    for (int g = 0; g < b->n_groups; ++g) {
        if (b->slabs[g].ncols == 0) continue;
        swept += 8.0 * (double)b->slabs[g].ncols * (double)b->m;
        cols += (double)b->slabs[g].ncols;
        ++groups;
    }
    cols /= std::max(1, groups);
    const EmCodesModel M = em_codes_decide(b, swept, cols, false, 14.0);
    for (int i = 0; i < 12; ++i) out[i] = 0.0;
    out[0] = M.direct_ms;
    out[1] = M.saves;
    out[2] = M.build_ms;
    out[3] = 14.0;
    out[4] = M.pays ? 1.0 : 0.0;
    out[9] = M.sampled ? 1.0 : 0.0;
    if (K_score > 0) {
        if (wgs_codes_scoring_model(b, K_score, &out[5], &out[6], &out[7])) out[8] = out[5] * (1.0 - out[6]) > out[7] ? 1.0 : 0.0;
        out[9] = 1.0;
    }
    if (b->plan.state != 0) {
        out[10] = b->plan.mean_l;
        out[11] = b->plan.mean_g;
    }
    return 0;
}

// The buffers of two iterations per sweep: a third frequency buffer and a second set of partial sums.  false: no memory for them.
static bool em_fuse_buffers(wgs_em *em)
{
    if (em->fbuf[2]) return true;
    const size_t fbytes = (size_t)em->n_fits * em->b->m * sizeof(float);
    const int64_t ntiles = wgs_ntiles(em->b->m);
    if (wgs_malloc(&em->fbuf[2], fbytes) != hipSuccess || wgs_malloc(&em->d_part_b, sizeof(double) * (size_t)em->n_fits * ntiles) != hipSuccess) {
        (void)hipGetLastError();
        if (em->fbuf[2]) (void)hipFree(em->fbuf[2]);
        em->fbuf[2] = nullptr;
        return false;
    }
    return true;
}

// What one sweep does, decided before anything of it is written or enqueued.
struct EmSweepPlan {
    std::vector<int32_t> order;                        // the fits in launch order: by slab when several share one
    bool shared = false;                               // several fits per slab: the group kernels, up to fits_per_group per group
    int fits_per_group = 1;
    wgs_codes *codes = nullptr;                        // the coded kernels read these; nullptr: the float32 slabs
    bool can_fuse = false;                             // this rank could run two iterations per sweep (what it tells the others)
    bool fusing = false;                               // it does, for the fits with (*may_fuse)[j] >= 2
    const std::vector<int32_t> *may_fuse = nullptr;
};

/* The plan of one sweep over the fits in `list`: which kernel, through the class codes or not, one iteration or two.  Fits of
 * different populations stream their slabs once (nontemporal loads); fits that share a slab (leave-one-out batches) are ordered by
 * slab and swept in groups per wavefront, which share the tile's loads and conversions.  May build the codes, run the sample pass and
 * allocate the buffers of fused sweeps, enqueues no sweep.  may_fuse[j] >= 2 (NULL: none): fit j may run two iterations. */
static EmSweepPlan em_plan_sweep(wgs_em *em, const std::vector<int32_t> &list, int sweeps_ahead, const std::vector<int32_t> *may_fuse,
                                 bool fuse_agreed, const EmSwitches &sw)
{
    wgs_beagle *b = em->b;
    EmSweepPlan p;
    double swept = 0.0, cols = 0.0;                    // (sums of integers: exact in any order)
    int fewest = INT32_MAX;
    std::vector<char> seen(b->n_groups, 0);
    for (int j : list) {
        const int g = em->group[j], ncols = b->slabs[g].ncols;
        p.shared = p.shared || seen[g];
        seen[g] = 1;
        swept += 8.0 * (double)ncols * (double)b->m;
        cols += (double)ncols;
        fewest = std::min(fewest, ncols);
    }
    cols /= (double)list.size();
    p.order = list;
    if (p.shared) std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t x, int32_t y) { return em->group[x] < em->group[y]; });
    // exact mode on a coded matrix: the sweep through the class codes (same frequencies, bit for bit)
    // -- leave-one-out batches (several fits per slab) where the table saves instructions (loo_codes_saving), else they stay with
    // em_sweep_group_kernel and its shared loads and conversions (also when the codes exist already: a scoring sweep may have built them)
    // -- and small populations stay with em_sweep_kernel too: below ~28 individuals the table costs more than it saves
    // (measured: 20 individuals 0.98x, 30 1.16x, 36 1.26x, 62 1.64x, 100 2.1x)
    // -- and the codes are BUILT for it only when the sweeps still to come repay the encode pass (em_codes_pay).
    // Codes that exist already (a scoring sweep built them, or wgs_beagle_codes_prepare) are used at once.
    const bool worth = em->mode == WGS_MODE_EXACT && sw.codes && (!p.shared || sw.loo_codes) && fewest >= sw.codes_min &&
                       (!p.shared || sw.sweeps_set || loo_codes_saving(wgs_beagle_codes_plan(b), cols) > 0.03);
    const bool build = worth && em_codes_pay(em, swept, cols, sweeps_ahead, p.shared, sw);
    {
        WGS_STALL_SCOPE("wgs_beagle_codes from the sweep");
        p.codes = worth ? wgs_beagle_codes(b, build, false) : nullptr;     // (memory not there yet: this sweep goes direct)
        if (p.codes && p.codes->lrows == 0 && p.codes->local_skipped && build) {
            // built by a scoring sweep, without the slabs' own numbering: this fit repays a full build
            const wgs_codes_plan keep = b->plan;
            wgs_beagle_drop_codes(b);
            b->plan = keep;
            p.codes = wgs_beagle_codes(b, true, false);
        }
    }
    WGS_STALL_SCOPE("the sweep's plan");
    if (p.codes && (p.codes->lrows == 0 || !em_coded_usable(b->ctx))) p.codes = nullptr;
    if (worth && !p.codes) ++b->direct_sweeps;          // (a sweep the codes could have served)
    // two iterations per sweep (em_kernels.hip: fused iterations): the coded sweep only, for the fits the caller allows (iterations
    // left, a place for the second sums); needs a third frequency buffer and a second set of partial sums, allocated on first use.
    // `can_fuse` is what THIS rank could do -- every input of it is rank-local (the codes' arrival, a cost model, environment
    // switches, free memory) -- and is what the rank tells the others (wgs_em_fit puts it into the sweep's collective); what the
    // sweep DOES additionally needs `fuse_agreed`: every rank has said it can.
    if (p.codes && may_fuse && sw.fuse && !p.shared) {    // (leave-one-out batches are bound by arithmetic: a second iteration that turns out unneeded is not free there)
        const bool wanted = std::any_of(p.order.begin(), p.order.end(), [&](int32_t j) { return (*may_fuse)[j] >= 2; });
        p.can_fuse = (em->fbuf[2] || wanted) && em_fuse_buffers(em);         // (no memory for the buffers: one iteration per sweep)
        p.fusing = p.can_fuse && wanted && (fuse_agreed || wgs_hook("em_fuse_without_agreement") != 0);
    }
    p.may_fuse = may_fuse;
    // groups of fits of one slab: four per wavefront for the float32 kernel (shared loads and conversions); through the codes a
    // wavefront walks up to 16 fits one after the other (the dictionary rows stay in registers)
    if (p.shared) p.fits_per_group = p.codes ? 16 : em_fits_per_group();
    return p;
}

// Where one sweep's descriptors and (first, count) group pairs are written (pinned host memory) and where they go on the device:
// a slot of the batch's own two-slot rings, or one of a longer ring whose owner enqueues many sweeps without waiting (wgs_em_stream).
struct EmDescSlot {
    FitDesc *h, *d;
    int32_t *hg, *dg;
};
static EmDescSlot em_ring_slot(wgs_em *em, int slot) { return EmDescSlot{em->h_descs[slot], em->d_descs[slot], em->h_groups[slot], em->d_groups[slot]}; }

// The slot's pinned memory from the plan: the fits' descriptors and the group table (returns its number of pairs); fuse_used,
// pend_cur / pend_prev.  ssq[j] receives fit j's sum, ssq_b[j] (NULL: ssq[j]) that of its second iteration; state (device, may be
// NULL) holds the fit states a sweep honours.
static int32_t em_write_descs(wgs_em *em, const EmSweepPlan &p, const EmDescSlot &slot, double *ssq, double *ssq_b, int32_t *state)
{
    const int64_t ntiles = wgs_ntiles(em->b->m);
    const int nb = em->fbuf[2] ? 3 : 2;
    for (size_t i = 0; i < p.order.size(); ++i) {
        const int j = p.order[i];
        const Slab &s = em->b->slabs[em->group[j]];
        FitDesc &d = slot.h[i];
        d.lcodes = p.codes ? p.codes->slabs[em->group[j]].lcodes : nullptr;
        d.ldict = p.codes ? p.codes->slabs[em->group[j]].ldict : nullptr;
        d.lrows = p.codes ? p.codes->lrows : 0;
        d.tile_rows = p.codes ? p.codes->slabs[em->group[j]].tile_rows : nullptr;
        d.nquads = p.codes ? p.codes->slabs[em->group[j]].nquads : 0;
        d.slab = s.base;
        const int fuse = p.fusing && (*p.may_fuse)[j] >= 2 ? 2 : 1;
        const EmBuffers first = em_rotate(em->cur[j], nb, 1), last = em_rotate(em->cur[j], nb, fuse);
        d.f_old = em_f(em, j, em->cur[j]);
        d.f_new = em_f(em, j, first.cur);
        d.f_new2 = em_f(em, j, last.cur);                    // (= f_new when one iteration runs)
        d.fuse = fuse;
        d.ssq = ssq + j;
        d.ssq2 = ssq_b ? ssq_b + j : d.ssq;
        d.ssq_part = em->d_part + (size_t)j * ntiles;
        d.ssq_part2 = fuse == 2 ? em->d_part_b + (size_t)j * ntiles : d.ssq_part;
        em->fuse_used[j] = (uint8_t)fuse;
        em->pend_cur[j] = last.cur;
        em->pend_prev[j] = last.prev;
        d.npairs = s.npairs;
        d.ncols = s.ncols;
        d.skip = em->skip_local[j];
        d.n_eff = em->n_eff[j];
        d.state = state ? state + j : nullptr;
    }
    int32_t n_groups = 0, *Hg = slot.hg;
    for (size_t i = 0; p.shared && i < p.order.size();) {
        size_t k = i + 1;
        while (k < p.order.size() && (int)(k - i) < p.fits_per_group && em->group[p.order[k]] == em->group[p.order[i]]) ++k;
        Hg[2 * n_groups] = (int32_t)i;
        Hg[2 * n_groups + 1] = (int32_t)(k - i);
        ++n_groups;
        i = k;
    }
    return n_groups;
}

/* Enqueue the planned sweep (+ the fixed-order reduction of its sums): descriptors into the slot's pinned memory and from
 * there to the device, then the plan's kernel in slices of fits or groups.  ev0 / ev1 (may be NULL) bracket the sweep kernel(s). */
static int em_enqueue_sweep(wgs_em *em, const EmSweepPlan &p, const EmDescSlot &slot, double *ssq, double *ssq_b, int32_t *state,
                            hipEvent_t ev0, hipEvent_t ev1)
{
    WGS_STALL_SCOPE("the sweep's launches");
    wgs_ctx *ctx = em->b->ctx;
    const int64_t m = em->b->m, ntiles = wgs_ntiles(m);
    const int32_t n_groups = em_write_descs(em, p, slot, ssq, ssq_b, state);
    FitDesc *D = slot.d;
    int32_t *Dg = slot.dg;
    // the slot's pinned memory stays untouched until the caller has waited for this sweep
    HIP_TRY(hipMemcpyAsync(D, slot.h, sizeof(FitDesc) * p.order.size(), hipMemcpyHostToDevice, ctx->stream));
    if (p.shared) HIP_TRY(hipMemcpyAsync(Dg, slot.hg, sizeof(int32_t) * 2 * n_groups, hipMemcpyHostToDevice, ctx->stream));
    ++em->sweep_paths[(p.codes ? 2 : 0) + (p.shared ? 1 : 0)];
    if (ev0) HIP_TRY(hipEventRecord(ev0, ctx->stream));
    // workgroups per fit / per group (at least one tile per workgroup for the coded kernels): slices stay below 2^31
    const int64_t per_unit = p.codes ? (ntiles + 7) / 8 * 8 + 8 : ((ntiles + 3) / 4 + 7) / 8 * 8 + 8;
    const size_t units = p.shared ? (size_t)n_groups : p.order.size();
    if (em_launch_sliced(units, (size_t)std::max<int64_t>(1, ((1ll << 31) - 1) / per_unit), [&](size_t off, int cnt) {
            if (p.codes && p.shared) return launch_em_coded_groups(ctx, D, Dg + 2 * off, cnt, m, p.codes->lrows);
            if (p.codes) return launch_em_coded(ctx, D + off, cnt, m, p.codes->lrows);
            if (p.shared) return launch_em_sweep_groups(ctx, D, Dg + 2 * off, cnt, m, em->mode);
            return launch_em_sweep(ctx, D + off, cnt, m, em->mode);
        }))
        return 1;
    if (ev1) HIP_TRY(hipEventRecord(ev1, ctx->stream));
    return em_launch_sliced(p.order.size(), 65535, [&](size_t off, int cnt) {
        double *part2 = em->d_part2 + off * ssq_reduce_chunks();
        return launch_ssq_reduce(ctx, D + off, cnt, m, part2) || (p.fusing && launch_ssq_reduce(ctx, D + off, cnt, m, part2, 1));
    });
}

// The sweep last enqueued for fit j has run: its new frequencies are current, prev holds the ones before.
static void em_commit_sweep(wgs_em *em, int j) { em->cur[j] = em->pend_cur[j]; em->prev[j] = em->pend_prev[j]; }

int wgs_em_step_dev(wgs_em *em, double *ssq_dev)
{
    WGS_REQUIRE(em && ssq_dev, "null argument");
    const EmSwitches sw;
    wgs_ctx *ctx = em->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    em->last.clear();
    for (int j = 0; j < em->n_fits; ++j)
        if (em->active[j]) em->last.push_back(j);
    HIP_TRY(hipMemsetAsync(ssq_dev, 0, sizeof(double) * em->n_fits, ctx->stream));
    if (em->last.empty()) return 0;
    em->step_slot ^= 1;         // (the slots alternate; the caller only starts the next step after consuming this step's sums)
    const EmSweepPlan p = em_plan_sweep(em, em->last, 0, nullptr, true, sw);
    if (em_enqueue_sweep(em, p, em_ring_slot(em, em->step_slot), ssq_dev, nullptr, nullptr, em->ev0, em->ev1)) return 1;
    for (int j : em->last) em_commit_sweep(em, j);
    return 0;
}

int wgs_em_step(wgs_em *em, double *ssq_host)
{
    WGS_REQUIRE(em, "null argument");
    if (wgs_em_step_dev(em, em->d_ssq)) return 1;
    wgs_ctx *ctx = em->b->ctx;
    if (ssq_host) {
        HIP_TRY(hipMemcpyAsync(ssq_host, em->d_ssq, sizeof(double) * em->n_fits, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int wgs_em_rmse_chain(wgs_em *em, int32_t fit, float carry_in, float *carry_out)
{
    WGS_REQUIRE(em && carry_out, "null argument");
    WGS_REQUIRE(fit >= 0 && fit < em->n_fits, "fit index out of range");
    wgs_ctx *ctx = em->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (launch_rmse_chain(ctx, em_f(em, fit, em->cur[fit]), em_f(em, fit, em->prev[fit]), em->b->m, carry_in, em->d_carry,
                          em->d_chain_work, reinterpret_cast<int *>(em->d_carry + 1)))
        return 1;
    float host[2];
    HIP_TRY(hipMemcpyAsync(host, em->d_carry, 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *carry_out = host[0];
    memcpy(&em->last_chain_serial_blocks, &host[1], sizeof(int));
    return 0;
}

/* ---- emMAF.py:15-27 for every fit of the batch in ONE call: wgs_em_fit enqueues sweep t (sweep, sum reduction, [RCCL all-reduce],
 * decision kernel, read-back) BEFORE it reads the decisions of sweep t-1, so the GPU never waits for the host.  What that takes in
 * bookkeeping -- who is listed, who really ran, who is parked for the exact chain -- is EmFitLedger's (em_fit_ledger.h, where the
 * protocol is described); here are the buffers, the chains and the loop that enqueues what the ledger says. */
// d_chain_out: a relay buffer of [n_fits] float32 carries | [n_fits] serial-block counts
static size_t em_chain_serial_off(size_t n) { return wgs_relay_bytes(sizeof(float) * n) / sizeof(float); }
static size_t em_chain_out_floats(size_t n) { return em_chain_serial_off(n) + n; }

static int em_fit_alloc(wgs_em *em)
{
    if (em->d_state) return 0;
    const size_t n = (size_t)em->n_fits;
    HIP_TRY(wgs_malloc(&em->d_state, sizeof(int32_t) * n));
    // (the sums of a sweep | its second iteration's | room for the rows the communicator attaches to their all-reduce)
    HIP_TRY(wgs_malloc(&em->d_ssq2, sizeof(double) * (2 * n + wgs_comm_tail_doubles())));
    HIP_TRY(hipMemset(em->d_ssq2, 0, sizeof(double) * (2 * n + wgs_comm_tail_doubles())));
    HIP_TRY(wgs_malloc(&em->d_jobs, sizeof(ChainJob) * n));
    HIP_TRY(wgs_malloc(&em->d_chain_out, sizeof(float) * em_chain_out_floats(n)));
    // workspace of the exact chains for all fits at once (60 bytes per fit and block of 4096 SNPs): no allocation
    // inside the convergence loop
    HIP_TRY(wgs_malloc(&em->d_chain_batch, rmse_chain_workspace_bytes(em->b->m) * n));
    em->chain_batch_jobs = n;
    HIP_TRY(hipHostMalloc(&em->h_jobs, sizeof(ChainJob) * n, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&em->h_chain_out, sizeof(float) * 2 * n, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&em->h_setstate, sizeof(int32_t) * n, hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipHostMalloc(&em->h_state[i], sizeof(int32_t) * n, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&em->h_ssq[i], sizeof(double) * (2 * n + wgs_comm_tail_doubles()), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&em->ev_it[i], hipEventDisableTiming));
    }
    return 0;
}

/* Exact chains of `fits` (all at once): converged[i] = the reference's `diff < tole` for fits[i]. */
static int em_resolve_chains(wgs_em *em, const std::vector<int32_t> &fits, double tole, int64_t m_total, wgs_comm *comm,
                             std::vector<char> &converged, int32_t generation, int32_t iteration)
{
    wgs_ctx *ctx = em->b->ctx;
    const int nj = (int)fits.size();
    converged.assign(nj, 0);
    if (nj == 0) return 0;
    for (int i = 0; i < nj; ++i) {
        const int j = fits[i];
        em->h_jobs[i] = ChainJob{em_f(em, j, em->cur[j]), em_f(em, j, em->prev[j]), 0.0f};
    }
    HIP_TRY(hipMemcpyAsync(em->d_jobs, em->h_jobs, sizeof(ChainJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    if (em_relay_chains(ctx, comm, WGS_OP_EM_CHAIN, generation, iteration, em->d_jobs, nj, em->b->m, em->d_chain_out, em->d_chain_batch,
                        reinterpret_cast<int *>(em->d_chain_out + em_chain_serial_off(em->n_fits)), em->h_chain_out))
        return 1;
    ++em->fit_chain_batches;
    for (int i = 0; i < nj; ++i) converged[i] = em_chain_converged(em->h_chain_out[i], m_total, tole);
    return 0;
}

int wgs_em_fit(wgs_em *em, int32_t max_iter, double tole, int64_t m_total, wgs_comm *comm, double guard_floor, int32_t *iters_out)
{
    WGS_REQUIRE(em && iters_out, "null argument");
    WGS_REQUIRE(m_total >= em->b->m, "m_total (%lld) is smaller than this shard (%lld SNPs)", (long long)m_total, (long long)em->b->m);
    const EmSwitches sw;
    wgs_ctx *ctx = em->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const EmBand band = em_band(tole, m_total, guard_floor);
    if (em_fit_alloc(em)) return 1;
    const int n = em->n_fits;
    // Across SNP shards every rank must run the same number of iterations per sweep (the sums of a sweep are all-reduced, and the
    // ledger counts iterations): two per sweep only once EVERY rank can -- its codes built with the slabs' own numbering
    // and the buffers at hand.  Whether a rank can is rank-local (its cost model, when its helper thread's allocation arrives, its
    // environment), so it is never acted upon directly: each sweep's all-reduce carries every rank's "I could" (the free word of its
    // tag row), the host reads the rows with the sweep's decisions -- one sweep behind, like everything else here -- and from then on
    // every rank fuses, at the same sweep.  A fit whose codes arrive during it on some rank therefore starts with one iteration per
    // sweep everywhere and switches to two everywhere.  The tag of the all-reduce also says how many fits the sweep lists and how
    // many EM iterations it runs; a rank that got this wrong is found at that very collective (rccl_comm.hip), not by its numbers.
    int world = 1, rank = 0;
    if (comm) wgs_comm_rank(comm, &rank, &world);
    const int32_t generation = comm ? wgs_comm_next_generation(comm) : 0;
    bool fuse_agreed = comm == nullptr;                      // one shard: nothing to agree on
    EmFitLedger ledger({em->cur, em->prev, em->pend_cur, em->pend_prev, em->fuse_used, em->active}, max_iter, iters_out);
    std::vector<char> conv;
    conv.reserve(n);
    {
        const std::vector<int32_t> init = ledger.initial_states();
        HIP_TRY(hipMemcpyAsync(em->d_state, init.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    em->fit_iterations = em->fit_chain_batches = 0;
    em->fit_sweep_ms = 0.0;
    em->fit_timed = 0;
    em->fit_sweep_pending = false;
    const auto t_begin = std::chrono::steady_clock::now();
    for (int t = 1;; ++t) {
        const int slot = t & 1;
        const bool read_back = ledger.in_flight();           // sweep t-1 was enqueued
        // ---- enqueue sweep t
        const std::vector<int32_t> &L = ledger.begin(t);
        if (ledger.in_flight()) {
            hipEvent_t sw0 = nullptr, sw1 = nullptr;         // this sweep's pair (the first EM_TIMED_SWEEPS sweeps of a fit are timed)
            if (em->fit_timed < EM_TIMED_SWEEPS) {
                while ((int)em->ev_sw.size() < 2 * em->fit_timed + 2) {
                    hipEvent_t e = nullptr;
                    HIP_TRY(hipEventCreate(&e));
                    em->ev_sw.push_back(e);
                }
                sw0 = em->ev_sw[2 * em->fit_timed];
                sw1 = em->ev_sw[2 * em->fit_timed + 1];
                ++em->fit_timed;
                em->fit_sweep_pending = true;
            }
            const EmSweepPlan p = em_plan_sweep(em, L, max_iter - t + 1, &ledger.may_fuse(), fuse_agreed, sw);
            if (em_enqueue_sweep(em, p, em_ring_slot(em, slot), em->d_ssq2, em->d_ssq2 + n, em->d_state, sw0, sw1)) return 1;
            // Fits that skipped this sweep have stale sums; the decision kernel ignores them, and they are stale
            // in the same way on every rank (all ranks take the same decisions).
            if (comm) {
                const wgs_coll_tag tag = {WGS_OP_EM_SUMS, generation, t, (int32_t)L.size(), ledger.iterations_listed(), p.can_fuse ? 1 : 0};
                if (wgs_comm_allreduce_tagged(comm, em->d_ssq2, 2 * n, &tag)) return 1;
            }
            if (launch_em_decide(ctx, em->d_descs[slot], (int)L.size(), band.lo, band.hi)) return 1;
            HIP_TRY(hipMemcpyAsync(em->h_state[slot], em->d_state, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipMemcpyAsync(em->h_ssq[slot], em->d_ssq2, sizeof(double) * (2 * n + (comm ? world * WGS_TAG_WORDS : 0)), hipMemcpyDeviceToHost,
                                   ctx->stream));
            HIP_TRY(hipEventRecord(em->ev_it[slot], ctx->stream));
            ++em->fit_iterations;
        }
        // ---- read the decisions of sweep t-1 while the GPU works on sweep t
        if (read_back) {
            const int ps = slot ^ 1;
            HIP_TRY(hipEventSynchronize(em->ev_it[ps]));     // also: the pinned descriptors of t-1 have been consumed
            if (comm) {
                if (wgs_comm_check(comm)) return 1;          // some rank's sweep t-1 was not this rank's sweep t-1
                bool all = true;                             // every rank's "I could run two iterations per sweep" as of sweep t-1
                for (int r = 0; r < world; ++r) all = all && em->h_ssq[ps][2 * n + r * WGS_TAG_WORDS + WGS_TAG_AUX] == 1.0;
                fuse_agreed = all;                           // acted upon from sweep t+1 on, by every rank alike
            }
            ledger.read(em->h_state[ps], em->h_ssq[ps] + n, band);
            while (!ledger.batch().empty()) {
                if (em_resolve_chains(em, ledger.batch(), tole, m_total, comm, conv, generation, ledger.batch_iteration())) return 1;
                // stream-ordered behind the sweep in flight (which must see these fits parked throughout)
                for (const EmStateWrite &w : ledger.resolved(conv)) {
                    em->h_setstate[w.fit] = w.state;
                    HIP_TRY(hipMemcpyAsync(em->d_state + w.fit, em->h_setstate + w.fit, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
                }
            }
        }
        if (!ledger.in_flight()) break;                      // nothing in flight: every fit finished or exhausted
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (comm) {
        // the ranks close the fit together: what each of them found (iteration counts, sweeps enqueued, chain resolutions) travels
        // as the tag of one last collective, so ranks that ended with different results fail here instead of returning them
        const EmClosing c = ledger.closing();
        const wgs_coll_tag tag = {WGS_OP_EM_FIT_END, generation, em->fit_iterations, c.sum, c.mix, em->fit_chain_batches};
        if (wgs_comm_allreduce_host_tagged(comm, nullptr, 0, &tag, nullptr)) return 1;
    }
    ledger.freeze_converged();
    em->fit_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    return 0;
}

/* Diagnostics of the last wgs_em_fit: iterations enqueued, batched exact-chain resolutions, wall seconds, and the
 * summed duration of its sweep kernels (HIP events on the context's stream around each iteration's sweep; read here, not
 * inside the fit; -1 while the codes' memory is being allocated on the helper thread -- the query would wait for it). */
int wgs_em_fit_stats(wgs_em *em, int32_t *iterations, int32_t *chain_batches, double *seconds, double *sweep_ms)
{
    WGS_REQUIRE(em, "null argument");
    if (iterations) *iterations = em->fit_iterations;
    if (chain_batches) *chain_batches = em->fit_chain_batches;
    if (seconds) *seconds = em->fit_seconds;
    if (sweep_ms) {
        if (em->fit_sweep_pending && em->b->ctx->allocs_in_flight.load() > 0) {
            *sweep_ms = -1.0;
            return 0;
        }
        if (em->fit_sweep_pending) {
            HIP_TRY(hipSetDevice(em->b->ctx->device));
            em->fit_sweep_ms = 0.0;
            for (int i = 0; i < em->fit_timed; ++i) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, em->ev_sw[2 * i], em->ev_sw[2 * i + 1]) == hipSuccess) em->fit_sweep_ms += ms;
            }
            (void)hipGetLastError();
            em->fit_sweep_pending = false;
        }
        *sweep_ms = em->fit_sweep_ms;
    }
    return 0;
}

int wgs_em_last_chain_serial_blocks(wgs_em *em) { return em ? em->last_chain_serial_blocks : -1; }

int wgs_debug_em_sweep_paths(wgs_em *em, int64_t counts[4])
{
    WGS_REQUIRE(em && counts, "null argument");
    for (int i = 0; i < 4; ++i) counts[i] = em->sweep_paths[i];
    return 0;
}

int wgs_em_last_sweep_ms(wgs_em *em, float *ms)
{
    WGS_REQUIRE(em && ms, "null argument");
    HIP_TRY(hipSetDevice(em->b->ctx->device));
    HIP_TRY(hipEventSynchronize(em->ev1));
    HIP_TRY(hipEventElapsedTime(ms, em->ev0, em->ev1));
    return 0;
}

int wgs_em_set_active(wgs_em *em, int32_t fit, int active)
{
    WGS_REQUIRE(em && fit >= 0 && fit < em->n_fits, "fit index out of range");
    em->active[fit] = active ? 1 : 0;
    return 0;
}

int wgs_em_n_active(wgs_em *em)
{
    int c = 0;
    for (int j = 0; j < em->n_fits; ++j) c += em->active[j];
    return c;
}

int wgs_em_clamp(wgs_em *em, int32_t fit, float lo, float hi)
{
    WGS_REQUIRE(em && fit >= 0 && fit < em->n_fits, "fit index out of range");
    HIP_TRY(hipSetDevice(em->b->ctx->device));
    return launch_clamp(em->b->ctx, em_f(em, fit, em->cur[fit]), em->b->m, lo, hi);
}

int wgs_em_get_f(wgs_em *em, int32_t fit, float *f_host)
{
    WGS_REQUIRE(em && f_host && fit >= 0 && fit < em->n_fits, "bad argument");
    HIP_TRY(hipSetDevice(em->b->ctx->device));
    HIP_TRY(hipMemcpyAsync(f_host, em_f(em, fit, em->cur[fit]), sizeof(float) * em->b->m, hipMemcpyDeviceToHost, em->b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(em->b->ctx->stream));
    return 0;
}

int wgs_em_get_f_range(wgs_em *em, int32_t fit, int previous, int64_t row0, int64_t nrows, float *f_host)
{
    WGS_REQUIRE(em && f_host && fit >= 0 && fit < em->n_fits, "bad argument");
    WGS_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= em->b->m, "row range [%lld, %lld) outside 0..%lld", (long long)row0,
                (long long)(row0 + nrows), (long long)em->b->m);
    if (nrows == 0) return 0;
    HIP_TRY(hipSetDevice(em->b->ctx->device));
    const float *src = em_f(em, fit, previous ? em->prev[fit] : em->cur[fit]) + row0;
    HIP_TRY(hipMemcpyAsync(f_host, src, sizeof(float) * nrows, hipMemcpyDeviceToHost, em->b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(em->b->ctx->stream));
    return 0;
}

int wgs_em_set_f(wgs_em *em, int32_t fit, const float *f_host)
{
    WGS_REQUIRE(em && f_host && fit >= 0 && fit < em->n_fits, "bad argument");
    HIP_TRY(hipSetDevice(em->b->ctx->device));
    HIP_TRY(hipMemcpyAsync(em_f(em, fit, em->cur[fit]), f_host, sizeof(float) * em->b->m, hipMemcpyHostToDevice, em->b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(em->b->ctx->stream));
    return 0;
}

const float *wgs_em_f_dev(wgs_em *em, int32_t fit)
{
    if (!em || fit < 0 || fit >= em->n_fits) return nullptr;
    return em_f(em, fit, em->cur[fit]);
}

/* ---- windowed fits: one GPU fits the sites of a file window by window ("the fit in windows").  The EM update
 * is per site; only the stopping test couples the sites, through one sum per iteration over ALL of them.  So a round pushes every
 * window of the file once, in file order, and each push runs the window's fits from 0.25 for as many iterations as the host asks:
 * the window's float64 sum of iteration t joins S[t][fit], the exact float32 chain of the (fit, iteration) pairs the host names goes
 * on from C[t][fit] -- the carry the window before left there, as a SNP shard's carry reaches the next shard (em_relay_chains) --
 * and fits whose stopping iteration is known stop there, are clamped and handed out.  S and C stay on the device from push to push;
 * the host reads them once per round (wgs_em_stream_read) and decides with the rule of wgs_em_fit (em_band / em_classify /
 * em_chain_converged; wgsassign_amd/windowed_fit.py keeps the rounds).  Nothing is read back while a window is fitted. */
constexpr int EM_STREAM_SLOTS = 256;    // sweeps a push enqueues before it waits for the device once (their descriptors stay pinned until then)
struct wgs_em_stream : StreamCursor {   // (pushed: in this round)
    int32_t n_fits = 0, max_iter = 0;
    int32_t rounds = 0;                 // rounds read so far
    double *d_S = nullptr;              // [max_iter][n_fits] sums of squared differences over the sites pushed in the accumulating round(s)
    float *d_C = nullptr;               // [max_iter][n_fits] float32 carries of the chains of this round
    double *d_win = nullptr;            // [n_fits] the sums of the sweep in flight
    int slots = 0;
    FitDesc *h_descs = nullptr, *d_descs = nullptr;        // [slots][n_fits]
    int32_t *h_groups = nullptr, *d_groups = nullptr;      // [slots][2 n_fits]
    size_t job_cap = 0;                 // chain jobs of one push
    ChainJob *h_jobs = nullptr, *d_jobs = nullptr;
    int32_t *h_cell = nullptr, *d_cell = nullptr;
    float *d_chain_out = nullptr;       // [n_fits]
    void *d_chain_work = nullptr;
    size_t chain_work_bytes = 0;
    int32_t *d_from = nullptr;          // [n_fits] wgs_em_stream_push_keep: the iterations of every fit whose sums S holds already
    // wgs_em_stream_push_masked: the compacted (f_t, f_t-1) of every fit over its kept sites of the window, [n_fits][stride] each, and
    // the compaction jobs of one push (one per chain job)
    float *d_ca = nullptr, *d_cb = nullptr;
    size_t compact_cap = 0;             // floats in each of the two
    size_t cjob_cap = 0;
    ZCompactJob *h_cjobs = nullptr, *d_cjobs = nullptr;
};

void wgs_em_stream_destroy(wgs_em_stream *st)
{
    if (!stream_retire(st)) return;
    for (void *p : {(void *)st->d_S, (void *)st->d_C, (void *)st->d_win, (void *)st->d_descs, (void *)st->d_groups, (void *)st->d_jobs,
                    (void *)st->d_cell, (void *)st->d_chain_out, st->d_chain_work, (void *)st->d_from, (void *)st->d_ca, (void *)st->d_cb, (void *)st->d_cjobs})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)st->h_descs, (void *)st->h_groups, (void *)st->h_jobs, (void *)st->h_cell, (void *)st->h_cjobs})
        if (p) (void)hipHostFree(p);
    delete st;
}

int wgs_em_stream_create(wgs_ctx *ctx, int32_t n_fits, int32_t max_iter, int64_t m_total, wgs_em_stream **out)
{
    WGS_REQUIRE(ctx && out, "null argument");
    WGS_REQUIRE(n_fits > 0 && max_iter >= 0 && m_total > 0, "a fit stream needs fits and sites (%d fits, %d iterations, %lld sites)", n_fits,
                max_iter, (long long)m_total);
    WGS_REQUIRE((int64_t)n_fits * std::max(1, max_iter) < (1ll << 30), "%d fits x %d iterations are too many for one fit stream", n_fits, max_iter);
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_em_stream *st = stream_new<wgs_em_stream>(ctx, m_total, WGS_LIVE_EM_STREAM);
    auto guard = on_failure([&] { wgs_em_stream_destroy(st); });
    st->n_fits = n_fits;
    st->max_iter = max_iter;
    const size_t n = (size_t)n_fits, cells = n * (size_t)std::max(1, max_iter);
    st->slots = std::max(1, std::min(max_iter, EM_STREAM_SLOTS));
    HIP_TRY(wgs_malloc(&st->d_S, sizeof(double) * cells));
    HIP_TRY(wgs_malloc(&st->d_C, sizeof(float) * cells));
    HIP_TRY(wgs_malloc(&st->d_win, sizeof(double) * n));
    HIP_TRY(wgs_malloc(&st->d_chain_out, sizeof(float) * n));
    HIP_TRY(wgs_malloc(&st->d_descs, sizeof(FitDesc) * n * st->slots));
    HIP_TRY(wgs_malloc(&st->d_groups, sizeof(int32_t) * 2 * n * st->slots));
    HIP_TRY(hipHostMalloc(&st->h_descs, sizeof(FitDesc) * n * st->slots, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&st->h_groups, sizeof(int32_t) * 2 * n * st->slots, hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(st->d_S, 0, sizeof(double) * cells, ctx->stream));
    HIP_TRY(hipMemsetAsync(st->d_C, 0, sizeof(float) * cells, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    *out = st;
    return 0;
}

// Room for the chain jobs of one push and for the workspace of the chains of one iteration (one per fit at most) over `m` sites.
static int em_stream_chain_room(wgs_em_stream *st, size_t jobs, int64_t m)
{
    wgs_ctx *ctx = st->ctx;
    if (jobs > st->job_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (void *p : {(void *)st->d_jobs, (void *)st->d_cell})
            if (p) HIP_TRY(hipFree(p));
        for (void *p : {(void *)st->h_jobs, (void *)st->h_cell})
            if (p) HIP_TRY(hipHostFree(p));
        st->d_jobs = st->h_jobs = nullptr;
        st->d_cell = st->h_cell = nullptr;
        st->job_cap = 0;
        const size_t cap = std::max(jobs, (size_t)st->n_fits * 8);
        HIP_TRY(wgs_malloc(&st->d_jobs, sizeof(ChainJob) * cap));
        HIP_TRY(wgs_malloc(&st->d_cell, sizeof(int32_t) * cap));
        HIP_TRY(hipHostMalloc(&st->h_jobs, sizeof(ChainJob) * cap, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&st->h_cell, sizeof(int32_t) * cap, hipHostMallocDefault));
        st->job_cap = cap;
    }
    const size_t work = rmse_chain_workspace_bytes(m) * (size_t)st->n_fits;
    if (jobs && work > st->chain_work_bytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (st->d_chain_work) HIP_TRY(hipFree(st->d_chain_work));
        st->d_chain_work = nullptr;
        st->chain_work_bytes = 0;
        HIP_TRY(wgs_malloc(&st->d_chain_work, work));
        st->chain_work_bytes = work;
    }
    return 0;
}

// Room for the compacted vectors of a masked push (2 x n_fits x stride floats, grown when a window keeps more) and for its compaction
// jobs (one per chain job).
static int em_stream_masked_room(wgs_em_stream *st, size_t jobs, int64_t stride)
{
    wgs_ctx *ctx = st->ctx;
    const size_t floats = (size_t)st->n_fits * (size_t)stride;
    if (floats > st->compact_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (void *p : {(void *)st->d_ca, (void *)st->d_cb})
            if (p) HIP_TRY(hipFree(p));
        st->d_ca = st->d_cb = nullptr;
        st->compact_cap = 0;
        if (wgs_malloc(&st->d_ca, sizeof(float) * floats) != hipSuccess || wgs_malloc(&st->d_cb, sizeof(float) * floats) != hipSuccess) {
            wgs_set_error("hipMalloc of 2 x %zu bytes for the compacted frequencies failed", sizeof(float) * floats);
            return 1;
        }
        st->compact_cap = floats;
    }
    if (jobs > st->cjob_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (st->d_cjobs) HIP_TRY(hipFree(st->d_cjobs));
        if (st->h_cjobs) HIP_TRY(hipHostFree(st->h_cjobs));
        st->d_cjobs = st->h_cjobs = nullptr;
        st->cjob_cap = 0;
        const size_t cap = std::max(jobs, (size_t)st->n_fits * 8);
        HIP_TRY(wgs_malloc(&st->d_cjobs, sizeof(ZCompactJob) * cap));
        HIP_TRY(hipHostMalloc(&st->h_cjobs, sizeof(ZCompactJob) * cap, hipHostMallocDefault));
        st->cjob_cap = cap;
    }
    return 0;
}

/* One window, through its EM batch `em` (made from the window matrix; one fit per fit of the stream).  The matrix's first site must
 * be the number of sites pushed in this round and a multiple of WGS_WINDOW_ALIGN, every window but the last holds a multiple of
 * WGS_WINDOW_ALIGN sites, and the batch has the stream's number of fits: anything else is refused before a kernel is launched.
 *   run_iters[fit]   iterations fit runs here from f = 0.25 (0 .. max_iter; 0: the fit is left alone unless it is final);
 *   final[fit]       (may be NULL) != 0: run_iters[fit] is the fit's stopping iteration -- afterwards its frequencies are clamped to
 *                    [clamp_lo[fit], clamp_hi[fit]] (WGSassign.py:236-240) and copied to f_out[fit * f_stride .. + window rows);
 *   chain_fit / chain_iter [n_chain]   the exact chain over (f_t, f_t-1) of this window for fit chain_fit[i], t = chain_iter[i]
 *                    (1 <= t <= run_iters[fit]; sorted by t), from C[t][fit] to C[t][fit];
 *   add_sums         != 0: the window's sum of every iteration t a fit runs is added to S[t][fit].
 * Returns when the device is done with the window: its matrix may be refilled, f_out holds the final fits' rows. */
// Both pushes.  keep: final fits are clamped and stay in the batch (no f_out); sums_from (keep only; may be NULL: no sums): the sum of
// iteration t of a fit joins S only for t > sums_from[fit].  zk / fit_slot (both or neither; wgs_em_stream_push_masked): the chain of a
// fit runs over the sites slot fit_slot[fit] of zk kept in this window -- (f_t, f_t-1) compacted in site order, every chain job of
// an iteration by ONE launch -- and a fit that kept nothing here leaves C[t][fit] as it is.
static int em_stream_push_window(wgs_em_stream *st, wgs_em *em, const int32_t *run_iters, const int32_t *final, const float *clamp_lo,
                                 const float *clamp_hi, const int32_t *chain_fit, const int32_t *chain_iter, int32_t n_chain, int add_sums,
                                 float *f_out, int64_t f_stride, bool keep, const int32_t *sums_from, wgs_zkeep *zk = nullptr,
                                 const int32_t *fit_slot = nullptr)
{
    WGS_REQUIRE(st && em && run_iters, "null argument");
    wgs_beagle *window = em->b;
    WGS_REQUIRE(window->ctx == st->ctx, "the window belongs to another context than the fit stream");
    WGS_REQUIRE(em->n_fits == st->n_fits, "the window's batch has %d fits, the fit stream %d", em->n_fits, st->n_fits);
    WGS_REQUIRE(em->mode == WGS_MODE_EXACT, "windowed fits are exact fits");
    const int n = st->n_fits;
    const int64_t m = window->m;
    int32_t T = 0;
    bool any_final = false;
    STREAM_TRY(em_stream_window_refusal(window->site0, m, em->cap_m, st->pushed, st->m_total, WGS_WINDOW_ALIGN, why, sizeof why) ||
               em_stream_plan_refusal(n, st->max_iter, run_iters, final, clamp_lo && clamp_hi, keep || f_out != nullptr, keep ? m : f_stride, m,
                                      chain_fit, chain_iter, n_chain, &T, &any_final, why, sizeof why) ||
               (sums_from && em_stream_sums_from_refusal(n, run_iters, sums_from, why, sizeof why)) ||
               (zk && em_stream_masked_refusal(window, zk->b, n, zk->count, fit_slot, why, sizeof why)));
    const EmSwitches sw;
    wgs_ctx *ctx = st->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (em_stream_chain_room(st, (size_t)n_chain, m)) return 1;
    const int64_t stride = zk ? em_stream_masked_stride(n, fit_slot, zk->total.data()) : 0;
    if (zk) {
        if (em_stream_masked_room(st, (size_t)n_chain, stride)) return 1;
        // what lies behind a fit's kept count stays 0 through every iteration of this push: (0 - 0)^2 adds nothing
        HIP_TRY(hipMemsetAsync(st->d_ca, 0, sizeof(float) * (size_t)n * stride, ctx->stream));
        HIP_TRY(hipMemsetAsync(st->d_cb, 0, sizeof(float) * (size_t)n * stride, ctx->stream));
    }
    if (sums_from) {
        if (!st->d_from) HIP_TRY(wgs_malloc(&st->d_from, sizeof(int32_t) * (size_t)n));
        HIP_TRY(hipMemcpyAsync(st->d_from, sums_from, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));          // (sums_from is the caller's)
    }
    if (st->pushed == 0)                                     // a round begins: its chains start from zero
        HIP_TRY(hipMemsetAsync(st->d_C, 0, sizeof(float) * (size_t)n * std::max(1, st->max_iter), ctx->stream));
    if (launch_fill(ctx, em->fbuf[0], (int64_t)n * m, 0.25f)) return 1;       // emMAF.py:17-18
    em->cur.assign(n, 0);
    em->prev.assign(n, 1);
    std::vector<int32_t> list;
    list.reserve(n);
    int next_chain = 0, n_jobs = 0;         // chains of the plan looked at; chain jobs written (fewer when a masked fit kept nothing here)
    for (int t = 1; t <= T; ++t) {
        const int s = (t - 1) % st->slots;
        if (t > 1 && s == 0) HIP_TRY(hipStreamSynchronize(ctx->stream));      // the ring of pinned descriptors goes round
        list.clear();
        for (int j = 0; j < n; ++j)
            if (t <= run_iters[j]) list.push_back(j);        // (a fit past its last iteration keeps the frequencies of that iteration)
        em->fit_iterations = t - 1;
        const EmSweepPlan p = em_plan_sweep(em, list, T - t + 1, nullptr, true, sw);
        const EmDescSlot slot = {st->h_descs + (size_t)s * n, st->d_descs + (size_t)s * n, st->h_groups + (size_t)s * 2 * n,
                                 st->d_groups + (size_t)s * 2 * n};
        HIP_TRY(hipMemsetAsync(st->d_win, 0, sizeof(double) * n, ctx->stream));
        if (em_enqueue_sweep(em, p, slot, st->d_win, nullptr, nullptr, nullptr, nullptr)) return 1;
        for (int j : list) em_commit_sweep(em, j);
        if (add_sums && !sums_from && launch_em_stream_add_sums(ctx, st->d_win, st->d_S + (size_t)(t - 1) * n, n)) return 1;
        if (sums_from && launch_em_stream_add_sums_above(ctx, st->d_win, st->d_S + (size_t)(t - 1) * n, st->d_from, t, n)) return 1;
        // the chains of iteration t, over what this sweep wrote and what it read
        const int first = n_jobs;
        while (next_chain < n_chain && chain_iter[next_chain] == t) {
            const int j = chain_fit[next_chain++];
            const float *cur = em_f(em, j, em->cur[j]), *prev = em_f(em, j, em->prev[j]);
            if (zk) {
                if (zk->total[fit_slot[j]] == 0) continue;   // nothing kept in this window: C[t][fit] is handed on bit for bit
                float *va = st->d_ca + (size_t)j * stride, *vb = st->d_cb + (size_t)j * stride;
                st->h_cjobs[n_jobs] = ZCompactJob{cur, prev, va, vb, fit_slot[j]};
                cur = va;
                prev = vb;
            }
            st->h_jobs[n_jobs] = ChainJob{cur, prev, 0.0f};
            st->h_cell[n_jobs] = (int32_t)((size_t)(t - 1) * n + j);
            ++n_jobs;
        }
        if (zk && n_jobs > first) {                          // every chain job of this iteration compacted by one launch
            HIP_TRY(hipMemcpyAsync(st->d_cjobs + first, st->h_cjobs + first, sizeof(ZCompactJob) * (n_jobs - first), hipMemcpyHostToDevice,
                                   ctx->stream));
            if (launch_zcompact(ctx, st->d_cjobs + first, n_jobs - first, m, zk->mask, zk->off)) return 1;
        }
        for (int i = first; i < n_jobs; i += n) {            // (at most one chain per fit shares the workspace)
            const int cnt = std::min(n, n_jobs - i);
            HIP_TRY(hipMemcpyAsync(st->d_jobs + i, st->h_jobs + i, sizeof(ChainJob) * cnt, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(st->d_cell + i, st->h_cell + i, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, ctx->stream));
            if (launch_em_stream_chain_load(ctx, st->d_jobs + i, st->d_cell + i, st->d_C, cnt)) return 1;
            if (launch_rmse_chain_batch(ctx, st->d_jobs + i, cnt, zk ? stride : m, st->d_chain_out, st->d_chain_work, nullptr)) return 1;
            if (launch_em_stream_chain_store(ctx, st->d_chain_out, st->d_cell + i, st->d_C, cnt)) return 1;
        }
    }
    for (int j = 0; j < n && any_final; ++j) {
        if (!final[j]) continue;
        float *f = em_f(em, j, em->cur[j]);
        if (launch_clamp(ctx, f, m, clamp_lo[j], clamp_hi[j])) return 1;
        if (!keep) HIP_TRY(hipMemcpyAsync(f_out + (size_t)j * f_stride, f, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st->pushed += m;
    return 0;
}

int wgs_em_stream_push(wgs_em_stream *st, wgs_em *em, const int32_t *run_iters, const int32_t *final, const float *clamp_lo,
                       const float *clamp_hi, const int32_t *chain_fit, const int32_t *chain_iter, int32_t n_chain, int add_sums,
                       float *f_out, int64_t f_stride)
{
    return em_stream_push_window(st, em, run_iters, final, clamp_lo, clamp_hi, chain_fit, chain_iter, n_chain, add_sums, f_out, f_stride, false,
                                 nullptr);
}

/* wgs_em_stream_push for fits nobody on the host wants (the leave-one-out re-fits, wgs_loo_stream_push): a final fit is clamped and
 * STAYS in the batch, where wgs_em_f_dev finds it until the batch is pushed again -- nothing of the window's size is copied anywhere.
 * sums_from (may be NULL: this push adds no sums): the window's sum of iteration t of a fit joins S[t][fit] for t > sums_from[fit]
 * only, 0 <= sums_from[fit] <= run_iters[fit] -- a round that runs a fit further than an earlier one did adds what is new and nothing
 * twice (S is zeroed when the stream is made and never again). */
int wgs_em_stream_push_keep(wgs_em_stream *st, wgs_em *em, const int32_t *run_iters, const int32_t *final, const float *clamp_lo,
                            const float *clamp_hi, const int32_t *chain_fit, const int32_t *chain_iter, int32_t n_chain,
                            const int32_t *sums_from)
{
    return em_stream_push_window(st, em, run_iters, final, clamp_lo, clamp_hi, chain_fit, chain_iter, n_chain, sums_from != nullptr, nullptr, 0,
                                 true, sums_from);
}

/* wgs_em_stream_push_keep with no sums for fits whose stopping test runs over a site subset (the masked leave-one-out fits of
 * --get_reference_z_score): the chain of (fit, t) runs over the sites slot fit_slot[fit] of `zk` kept in this window, from C[t][fit] to
 * C[t][fit]; a fit that kept nothing here hands its carry on.  Nothing joins S, nothing is read back between the iterations. */
int wgs_em_stream_push_masked(wgs_em_stream *st, wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, const int32_t *run_iters,
                              const int32_t *final, const float *clamp_lo, const float *clamp_hi, const int32_t *chain_fit,
                              const int32_t *chain_iter, int32_t n_chain)
{
    WGS_REQUIRE(zk, "null argument");
    return em_stream_push_window(st, em, run_iters, final, clamp_lo, clamp_hi, chain_fit, chain_iter, n_chain, 0, nullptr, 0, true, nullptr, zk,
                                 fit_slot);
}

/* The round's one read-back: S (max_iter x n_fits float64) and C (max_iter x n_fits float32), either may be NULL.  rc 2 before all
 * m_total sites were pushed; afterwards the next round begins at site 0. */
int wgs_em_stream_read(wgs_em_stream *st, double *S_host, float *C_host)
{
    WGS_REQUIRE(st, "null argument");
    STREAM_TRY(stream_all_pushed_refusal(st->pushed, st->m_total, why, sizeof why));
    HIP_TRY(hipSetDevice(st->ctx->device));
    const size_t cells = (size_t)st->n_fits * st->max_iter;
    if (S_host && cells) HIP_TRY(hipMemcpyAsync(S_host, st->d_S, sizeof(double) * cells, hipMemcpyDeviceToHost, st->ctx->stream));
    if (C_host && cells) HIP_TRY(hipMemcpyAsync(C_host, st->d_C, sizeof(float) * cells, hipMemcpyDeviceToHost, st->ctx->stream));
    HIP_TRY(hipStreamSynchronize(st->ctx->stream));
    st->pushed = 0;
    ++st->rounds;
    return 0;
}

}   // extern "C"
