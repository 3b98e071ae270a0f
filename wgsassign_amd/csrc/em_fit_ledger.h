// The bookkeeping of wgs_em_fit (em_api.hip), host-only and free of HIP: the convergence rule, the rotation of a fit's frequency
// buffers, the reference's stopping test, and EmFitLedger -- which fit is listed for which sweep, how many iterations it has run,
// which fits are parked for the exact chain and what becomes of them.  Pure integer logic over what the device reports, so a
// stand-alone program drives it on the CPU against a model of the device (tests/c_abi/em_fit_ledger_check.cpp).
// Standard headers only; em_classify / em_decide are also what em_decide_kernel (em_kernels.hip) runs.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define EM_HOST_DEVICE __host__ __device__
#else
#define EM_HOST_DEVICE
#endif

// A fit's state on the device.  A sweep skips every fit that is not EM_ACTIVE.  A fused sweep runs two iterations, and the first
// decides first: _A says that the FIRST of the two converged / is undecided (the second is then dropped, or counts only once the
// exact chain has said that the first goes on); the plain values of a fused sweep speak of the second.
enum { EM_ACTIVE = 0, EM_CONVERGED = 1, EM_UNDECIDED = 2, EM_CONVERGED_A = 3, EM_UNDECIDED_A = 4 };

/* ---- the convergence rule: emMAF.py:22-23 from a float64 sum of squared differences.  The sum decides `diff < tole` unless it lies
 * in the band [lo, hi) around tole^2 * m in which the reference's serial float32 sum may fall on either side; device.py has the same
 * rule as guard_band / decide_converged (and the reasoning behind the band's width) for the ranks that run the Python protocol. */
struct EmBand {
    double lo, hi;
};

inline EmBand em_band(double tole, int64_t m_total, double guard_floor)
{
    EmBand band = {-1.0, -INFINITY};                         // tole <= 0 or NaN: `diff < tole` never holds
    if (tole > 0) {
        const double thresh = tole * tole * (double)m_total;
        const double rounding = (double)m_total * 0x1p-24;
        const double g = (guard_floor > rounding ? guard_floor : rounding) + 1e-6;
        band.lo = g < 1.0 ? thresh * (1.0 - g) : -1.0;
        band.hi = thresh * (1.0 + g);
    }
    return band;
}

// EM_CONVERGED below the band, EM_ACTIVE (goes on) at or above it, EM_UNDECIDED inside.  NaN never converges (NaN < tole is False).
EM_HOST_DEVICE inline int em_classify(double sum, EmBand band)
{
    return (sum != sum || sum >= band.hi) ? EM_ACTIVE : (sum < band.lo ? EM_CONVERGED : EM_UNDECIDED);
}

// The state an active fit gets from the sums of a sweep of `fuse` iterations: of two, the first decides first, and only when it
// goes on does the second count.
EM_HOST_DEVICE inline int em_decide(double ssq_first, double ssq_second, int fuse, EmBand band)
{
    const int first = em_classify(ssq_first, band);
    if (fuse != 2) return first;
    if (first == EM_CONVERGED) return EM_CONVERGED_A;
    if (first == EM_UNDECIDED) return EM_UNDECIDED_A;
    return em_classify(ssq_second, band);
}

// The reference's stopping test on the serial float32 sum `carry` over n SNPs (device.py: chain_diff(...) < tole).
inline bool em_chain_converged(float carry, int64_t n, double tole)
{
    const float res = carry / (float)n;                      // emMAF_cy.pyx:32
    return sqrt((double)res) < tole;                         // emMAF_cy.pyx:33, emMAF.py:23
}

/* ---- the rotation of a fit's frequency buffers: `cur` holds the current frequencies, `prev` the ones an iteration earlier. */
struct EmBuffers {
    uint8_t cur, prev;
};

// Where cur / prev point after a sweep of `fuse` iterations that starts from buffer `cur` of `nb`: every iteration writes the next
// buffer round the ring (two iterations need nb = 3: the second must not overwrite what the first reads).
inline EmBuffers em_rotate(int cur, int nb, int fuse) { return EmBuffers{(uint8_t)((cur + fuse) % nb), (uint8_t)((cur + fuse - 1) % nb)}; }

// The inverse step for a sweep of two iterations over three buffers: the view in which the FIRST iteration is the result (its
// frequencies in cur, the sweep's input in prev).  em_rotate(view.cur, 3, 1) leads back to `after`.
inline EmBuffers em_first_of_two(EmBuffers after) { return EmBuffers{after.prev, (uint8_t)(3 - after.cur - after.prev)}; }

/* ---- the ledger of one wgs_em_fit call.
 * The host enqueues sweep t (sweep, sum reduction, [all-reduce], decision kernel, read-back of states and sums) BEFORE it reads the
 * decisions of sweep t-1, so the GPU never waits for the host:
 *   - the decision kernel settles the clear cases on the device and parks the fits whose sum lies in the band;
 *   - a sweep skips every fit that is not EM_ACTIVE, so a fit that converged at t-1 keeps the frequencies of update t-1 (emMAF.py:23-25
 *     breaks after the update) and a parked fit keeps both vectors its exact chain needs;
 *   - the host, one sweep behind, resolves parked fits with the exact serial float32 chain (a batch at a time) and either finishes
 *     them or re-activates them -- such a fit simply runs its next sweep one sweep later.
 * So when sweep t is listed, the ledger knows the decisions of t-2 only: a fit listed for t may turn out to have finished or been
 * parked at t-1; its sweep t then returned at once and must not be counted (`skipped`).  Who really ran t-1 is exact at begin(t):
 * the list of t-1 minus the fits marked when the decisions of t-2 were read.
 * Everything here follows from all-reduced sums and relayed carries alone, so every rank's ledger takes the same path; closing()
 * is what the ranks compare at the end.
 *
 * One call goes: begin(1), [enqueue], begin(2), [enqueue], read(of 1), {batch(), resolved()}*, begin(3), [enqueue], read(of 2), ...
 * until a begin() lists nothing (in_flight() false).  It borrows the fits' buffer positions and the sweep last enqueued for each
 * (cur / prev / pend_cur / pend_prev / fuse_used: whoever writes a sweep's descriptors sets the last three) and `active`. */
struct EmStateWrite {
    int32_t fit, state;
};

struct EmClosing {
    int32_t sum, mix;
};

class EmFitLedger {
public:
    struct Fits {
        std::vector<uint8_t> &cur, &prev, &pend_cur, &pend_prev, &fuse_used, &active;
    };

    // iters_out[n]: per fit the iteration it converged at, 0 while it has not (and for good when it exhausts max_iter: the
    // reference prints nothing then).  Every vector gets its full size here: nothing below allocates.
    EmFitLedger(Fits fits, int32_t max_iter, int32_t *iters_out)
        : f_(fits), n_((int)fits.active.size()), max_iter_(max_iter), iters_(iters_out), fin_(n_), skipped_(n_, 0), sweeps_(n_, 0), may_fuse_(n_, 1)
    {
        for (std::vector<int32_t> *v : {&lists_[0], &lists_[1], &ran_, &parked_, &parked_a_}) v->reserve(n_);
        writes_.reserve(n_);
        for (int j = 0; j < n_; ++j) {
            iters_[j] = 0;
            fin_[j] = !f_.active[j];
        }
    }

    // The device states the fit starts from: a fit that is not active never sweeps.
    std::vector<int32_t> initial_states() const
    {
        std::vector<int32_t> init(n_);
        for (int j = 0; j < n_; ++j) init[j] = f_.active[j] ? EM_ACTIVE : EM_CONVERGED;
        return init;
    }

    // Commits sweep t-1 for the fits that really ran it and lists sweep t: every unfinished fit with iterations left (fits that
    // turn out to have converged at t-1 return at once).  may_fuse()[j] >= 2: fit j has room for two iterations.
    const std::vector<int32_t> &begin(int t)
    {
        t_ = t;
        ran_.clear();
        for (int32_t j : lists_[(t & 1) ^ 1]) {
            if (skipped_[j]) continue;
            sweeps_[j] += f_.fuse_used[j];                   // one EM iteration, or the two of a fused sweep
            f_.cur[j] = f_.pend_cur[j];
            f_.prev[j] = f_.pend_prev[j];
            ran_.push_back(j);
        }
        skipped_.assign(n_, 0);
        std::vector<int32_t> &list = lists_[t & 1];
        list.clear();
        for (int j = 0; j < n_; ++j) {
            if (!fin_[j] && sweeps_[j] < max_iter_) list.push_back(j);
            may_fuse_[j] = max_iter_ - sweeps_[j] >= 2 ? 2 : 1;        // (an odd limit ends with a one-iteration sweep)
        }
        return list;
    }
    const std::vector<int32_t> &may_fuse() const { return may_fuse_; }

    // Whether the sweep of the last begin() lists any fit; false ends the call: every fit finished or exhausted.
    bool in_flight() const { return !lists_[t_ & 1].empty(); }

    // EM iterations of the sweep just enqueued (its descriptors written: fuse_used), for the collective's tag.
    int32_t iterations_listed() const
    {
        int32_t sum = 0;
        for (int32_t j : lists_[t_ & 1]) sum += f_.fuse_used[j];
        return sum;
    }

    // Consumes the read-back of sweep t-1 (states[n]; second_sums[n]: the all-reduced sums of second iterations, which must stay
    // readable until the batches are resolved) after sweep t has been enqueued: finishes, steps back or exhausts the fits that ran
    // and parks the undecided ones, all of them marked so that their sweep t is not counted.  Then batch() is the first chain batch.
    void read(const int32_t *states, const double *second_sums, EmBand band)
    {
        second_sums_ = second_sums;
        band_ = band;
        parked_.clear();
        parked_a_.clear();
        for (int32_t j : ran_) {
            switch (states[j]) {
            case EM_CONVERGED:
                skipped_[j] = 1;
                finish(j);
                break;
            case EM_CONVERGED_A:                             // the first iteration's frequencies are the result, the second is dropped
                skipped_[j] = 1;
                view_first_of_two(j);
                sweeps_[j] -= 1;
                finish(j);
                break;
            case EM_UNDECIDED:
                skipped_[j] = 1;
                parked_.push_back(j);
                break;
            case EM_UNDECIDED_A:                             // the exact chain speaks about (f_a, f_in): cur / prev show them for the call
                skipped_[j] = 1;
                view_first_of_two(j);
                parked_a_.push_back(j);
                break;
            default:
                if (sweeps_[j] >= max_iter_) fin_[j] = 1;    // exhausted: the reference prints nothing, iters stays 0
            }
        }
        stage_ = !parked_a_.empty() ? STAGE_A : !parked_.empty() ? STAGE_PLAIN : STAGE_NONE;
    }

    // The fits whose exact chain over (cur, prev) is to be resolved now (empty: none left), and the iteration number of the
    // batch's collectives: the _A batch of sweep t travels as 2t, the plain one as 2t + 1.
    const std::vector<int32_t> &batch() const { return stage_ == STAGE_A ? parked_a_ : stage_ == STAGE_PLAIN ? parked_ : none_; }
    int32_t batch_iteration() const { return 2 * t_ + (stage_ == STAGE_PLAIN ? 1 : 0); }

    // Applies the verdicts of batch() (converged[i] for its fit i) and moves on to the next batch.  Returns the device states to
    // write, in order, stream-ordered behind the sweep in flight (which must see these fits parked throughout).
    const std::vector<EmStateWrite> &resolved(const std::vector<char> &converged)
    {
        writes_.clear();
        if (stage_ == STAGE_A) {
            for (size_t i = 0; i < parked_a_.size(); ++i) {
                const int32_t j = parked_a_[i];
                if (converged[i]) {
                    sweeps_[j] -= 1;
                    finish(j);
                    writes_.push_back({j, EM_CONVERGED});
                    continue;
                }
                // the first iteration goes on, so the second one's result stands and its sum is classified here as the device
                // would have (the same band on the same all-reduced float64), possibly parking the fit again
                const EmBuffers b = em_rotate(f_.cur[j], 3, 1);
                f_.cur[j] = b.cur;
                f_.prev[j] = b.prev;
                const int second = em_classify(second_sums_[j], band_);
                if (second == EM_UNDECIDED) {
                    parked_.push_back(j);
                    continue;
                }
                if (second == EM_CONVERGED) finish(j);
                else if (sweeps_[j] >= max_iter_) fin_[j] = 1;
                writes_.push_back({j, fin_[j] ? EM_CONVERGED : EM_ACTIVE});      // (exhausted: never swept again)
            }
            stage_ = !parked_.empty() ? STAGE_PLAIN : STAGE_NONE;
        } else if (stage_ == STAGE_PLAIN) {
            for (size_t i = 0; i < parked_.size(); ++i) {
                const int32_t j = parked_[i];
                if (converged[i]) finish(j);
                else if (sweeps_[j] >= max_iter_) fin_[j] = 1;
                writes_.push_back({j, converged[i] ? EM_CONVERGED : EM_ACTIVE});
            }
            stage_ = STAGE_NONE;
        }
        return writes_;
    }

    // What this rank found, for the tag of the collective that closes the fit: ranks that ended with different iteration counts
    // differ here.
    EmClosing closing() const
    {
        int64_t sum = 0, mix = 0;
        for (int j = 0; j < n_; ++j) {
            sum += iters_[j];
            mix = (mix * 31 + iters_[j] + 7 * (j + 1)) % 16777213;
        }
        return EmClosing{(int32_t)(sum % 16777213), (int32_t)mix};
    }

    // The fits that converged are frozen, as wgs_em_set_active(j, 0) would.
    void freeze_converged()
    {
        for (int j = 0; j < n_; ++j)
            if (iters_[j] > 0) f_.active[j] = 0;
    }

private:
    enum Stage { STAGE_NONE, STAGE_A, STAGE_PLAIN };

    // the fit ends with the frequencies in `cur`, sweeps_[j] iterations after its start
    void finish(int32_t j)
    {
        fin_[j] = 1;
        iters_[j] = sweeps_[j];
    }
    void view_first_of_two(int32_t j)
    {
        const EmBuffers b = em_first_of_two(EmBuffers{f_.cur[j], f_.prev[j]});
        f_.cur[j] = b.cur;
        f_.prev[j] = b.prev;
    }

    Fits f_;
    int n_;
    int32_t max_iter_;
    int32_t *iters_;
    int t_ = 0;
    std::vector<char> fin_, skipped_;                  // finished or exhausted | listed for the sweep in flight, which returned at once
    std::vector<int32_t> sweeps_, may_fuse_;           // EM iterations run so far
    std::vector<int32_t> lists_[2], ran_;              // the fits listed for sweep t (slot t & 1) and t-1 | those that ran t-1
    std::vector<int32_t> parked_, parked_a_, none_;
    std::vector<EmStateWrite> writes_;
    Stage stage_ = STAGE_NONE;
    const double *second_sums_ = nullptr;
    EmBand band_ = {-1.0, -INFINITY};
};
