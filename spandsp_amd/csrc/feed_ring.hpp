// feed_ring.hpp -- the bookkeeping of a pipelined feed's ring of slots (feed_api.hip), and the one tick loop of the three
// spangpu_*feed_run() calls.  No HIP in here: a ring is two counters and a flag per slot, and a host program can include this
// header alone (tests/c_callers/feed_ring.cpp does, under the sanitizers).
//
// Ticks are committed and collected in order: tick number t lives in slot t % depth from its commit to its collect.  A slot
// is busy between the two; n_commit - n_collect ticks are outstanding, at most `depth`.
#pragma once

#include <time.h>

#include "../../include/spangpu.h"

extern "C" int spangpu_set_error(int code, const char *msg);

namespace spg __attribute__((visibility("hidden")))
{

enum { kFeedMaxDepth = 8 };

struct FeedRing
{
    int depth;
    long long n_commit;
    long long n_collect;
    bool busy[kFeedMaxDepth];
};

static inline bool ring_depth_ok(int depth)
{
    return depth >= 1  &&  depth <= kFeedMaxDepth;
}

static inline int ring_outstanding(const FeedRing *r)
{
    return (int) (r->n_commit - r->n_collect);
}

// The slot the next commit takes, or SPANGPU_ERR_STATE while it still holds a tick (then every slot does).
static inline int ring_next(const FeedRing *r)
{
    const int slot = (int) (r->n_commit % r->depth);
    if (r->busy[slot])
        return spangpu_set_error(SPANGPU_ERR_STATE, "every slot of the feed holds a tick: collect one first");
    return slot;
}

// The last act of a commit: whatever fails before it leaves the ring as it was.
static inline void ring_committed(FeedRing *r, int slot)
{
    r->busy[slot] = true;
    r->n_commit++;
}

// The slot of the oldest tick not yet collected, -1 when none is outstanding.
static inline int ring_oldest(const FeedRing *r)
{
    return (r->n_collect < r->n_commit)  ?  (int) (r->n_collect % r->depth)  :  -1;
}

static inline void ring_collected(FeedRing *r, int slot)
{
    r->busy[slot] = false;
    r->n_collect++;
}

// A caller's tick loop, for measurements: `ticks` x { is the next slot free, commit(), collect() while more than `lag` ticks
// are outstanding }, then collect() until none is.  commit() and collect() are the family's own (what a collected tick is
// looked at for stays in collect()); both return < 0 to end the loop with that code.  *elapsed_ms = wall time of the whole
// loop, written on success only.  r == NULL is refused like the other bad arguments.
//
// A caller may know this loop in one of two other forms (the feeds' own tests write out the first):
//     for (i = 0; i < ticks; i++) { acquire; commit; if (outstanding > lag) collect; }    while (outstanding > 0) collect;
//     for (i = 0; i <= ticks; i++) { if (i < ticks) { acquire; commit; }    while (outstanding > (i < ticks ? lag : 0)) collect; }
// They make the same calls in the same order, and so does the loop below.  Nothing is outstanding at entry and a round commits
// one tick, so by induction at most lag + 1 are outstanding behind a commit: the `while` above `lag` runs once or not at all,
// which is the `if`.  The second form's round i == ticks commits nothing and collects down to none: the draining `while`.
// lag < depth is what keeps "is the next slot free" from ever refusing: behind a round at most `lag` slots are busy.
template <typename Commit, typename Collect>
static inline int ring_run(FeedRing *r, int ticks, int lag, double *elapsed_ms, Commit commit, Collect collect)
{
    if (r == nullptr  ||  ticks <= 0  ||  lag < 1  ||  lag >= r->depth  ||  ring_outstanding(r) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (lag in 1 .. depth - 1, nothing outstanding)");
    struct timespec t0, t1;
    int rc;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int i = 0;  i < ticks;  i++)
    {
        if ((rc = ring_next(r)) < 0  ||  (rc = commit()) < 0)
            return rc;
        while (ring_outstanding(r) > lag)
        {
            if ((rc = collect()) < 0)
                return rc;
        }
    }
    while (ring_outstanding(r) > 0)
    {
        if ((rc = collect()) < 0)
            return rc;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (elapsed_ms)
        *elapsed_ms = (t1.tv_sec - t0.tv_sec)*1e3 + (t1.tv_nsec - t0.tv_nsec)*1e-6;
    return SPANGPU_OK;
}

}   // namespace spg
