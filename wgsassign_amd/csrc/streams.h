// What the windowed streams (wgs_score_stream, wgs_em_stream, wgs_loo_stream, wgs_fisher_stream) share on the
// device side: where a stream stands in its file, the pair of device totals a push reads and writes, and the kinds of the
// live-object registry.  What a push refuses is host-only, in stream_checks.h.
#pragma once
#include "common.h"

// Every kind of the live-object registry (api.hip: wgs_live_*) above common.h's WGS_LIVE_EM = 1 and WGS_LIVE_SCORE = 2.  The depth
// table and the kept-site sets have parents and go with them; the streams and wgs_zsum have none, only their liveness is kept.
enum {
    WGS_LIVE_DEPTH = 3,
    WGS_LIVE_ZKEEP,
    WGS_LIVE_SCORE_STREAM,
    WGS_LIVE_EM_STREAM,
    WGS_LIVE_LOO_STREAM,
    WGS_LIVE_FISHER_STREAM,
    WGS_LIVE_ZSUM
};

// The refusals of stream_checks.h at work: `refusals` is a chain of them joined by ||, each writing into `why`; the first that
// refuses ends the call with rc 2 and its reason as the library's error.
#define STREAM_TRY(refusals)               \
    do {                                   \
        char why[256];                     \
        if (refusals) {                    \
            wgs_set_error("%s", why);      \
            return 2;                      \
        }                                  \
    } while (0)

// Where a stream stands: every stream struct derives from it.
struct StreamCursor {
    wgs_ctx *ctx = nullptr;
    int device = 0;
    int64_t m_total = 0, pushed = 0;    // sites of the file (of a round), and those pushed so far
};

// A new stream of type S on ctx's device, registered as alive; wgs_*_stream_create goes on under a guard that destroys it.
template <typename S>
static inline S *stream_new(wgs_ctx *ctx, int64_t m_total, int kind)
{
    S *st = new S();
    st->ctx = ctx;
    st->device = ctx->device;
    st->m_total = m_total;
    wgs_live_add(st, kind, nullptr);
    return st;
}

// The head of every wgs_*_stream_destroy: false when there is nothing to release (null, or destroyed already); else the stream's
// device is current and the caller frees what the stream owns -- plain allocations, not the context's pool, since the handle may
// outlive its context -- and deletes it.
template <typename S>
static inline bool stream_retire(S *st)
{
    if (!st || !wgs_live_remove(st)) return false;
    (void)hipSetDevice(st->device);
    return true;
}

// A running total kept on the device from push to push in two buffers in alternation: a kernel reads one and writes the other.
template <typename T>
struct RunningPair {
    T *buf[2] = {nullptr, nullptr};
    int cur = 0;                                    // buf[cur]: the totals over what was pushed so far
    hipError_t allocate(size_t count)
    {
        for (T *&p : buf)
            if (hipError_t e = wgs_malloc(&p, sizeof(T) * count)) return e;
        return hipSuccess;
    }
    T *current() const { return buf[cur]; }
    const T *before(bool any) const { return any ? buf[cur] : nullptr; }   // the totals before this window, or null: it is the first
    T *next() const { return buf[cur ^ 1]; }        // where this window's totals go
    void flip() { cur ^= 1; }
    void release()
    {
        for (T *p : buf)
            if (p) (void)hipFree(p);
    }
};
