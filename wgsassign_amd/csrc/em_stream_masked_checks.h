// What wgs_em_stream_push_masked (em_api.hip) refuses before it launches anything, beyond what every push refuses
// (em_stream_checks.h), and how much room its compacted vectors take: host-only and free of HIP, standard headers only, so a
// stand-alone program drives it on the CPU under the sanitizers (tests/c_abi/em_stream_masked_checks_check.cpp).
#pragma once
#include "em_stream_checks.h"

constexpr int32_t EM_STREAM_MASKED_MAX_FITS = 65535;      // the compaction of one iteration is ONE launch: one grid row per fit

// The kept-site set of a masked push: made from the batch's own matrix (the pointers are only compared), `keep_count` slots of
// which fit j takes fit_slot[j].  Returns 0, or 2 with the reason in msg.
inline int em_stream_masked_refusal(const void *batch_matrix, const void *keep_matrix, int32_t n_fits, int32_t keep_count,
                                    const int32_t *fit_slot, char *msg, size_t msg_len)
{
    EM_STREAM_REFUSE(fit_slot, "a masked push needs the slot of every fit");
    EM_STREAM_REFUSE(batch_matrix == keep_matrix, "the EM batch and the kept-site set belong to different matrices");
    EM_STREAM_REFUSE(n_fits <= EM_STREAM_MASKED_MAX_FITS, "a masked push holds at most %d fits, not %d", EM_STREAM_MASKED_MAX_FITS, n_fits);
    for (int32_t j = 0; j < n_fits; ++j)
        EM_STREAM_REFUSE(fit_slot[j] >= 0 && fit_slot[j] < keep_count, "fit %d: slot %d outside the kept-site set", j, fit_slot[j]);
    return 0;
}

// Floats per fit of each of the two compacted vectors: the largest kept count of this window among the fits' slots, at least 1
// (kept[s]: the sites slot s kept; the slots were checked by em_stream_masked_refusal).
inline int64_t em_stream_masked_stride(int32_t n_fits, const int32_t *fit_slot, const int64_t *kept)
{
    int64_t stride = 1;
    for (int32_t j = 0; j < n_fits; ++j)
        if (kept[fit_slot[j]] > stride) stride = kept[fit_slot[j]];
    return stride;
}
