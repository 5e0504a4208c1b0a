// feed_ring.cpp -- spandsp_amd/csrc/feed_ring.hpp on its own, on the host (tests/test_feed_ring.py builds this under
// -fsanitize=address,undefined and reads the transcript).  The ring's tick loop runs over stand-in commit / collect
// callables that print the slot they are given; then every refusal, with the code, the text and what the ring holds after.
#include <stdio.h>
#include <string.h>

#include "feed_ring.hpp"

using namespace spg;

static char last_error[128];

extern "C" int spangpu_set_error(int code, const char *msg)
{
    snprintf(last_error, sizeof(last_error), "%s", msg);
    return code;
}

// what a family's commit and collect do with the ring, and no more
static int commit(FeedRing *r)
{
    const int slot = ring_next(r);
    if (slot < 0)
        return slot;
    printf("commit %d\n", slot);
    ring_committed(r, slot);
    return SPANGPU_OK;
}

static int collect(FeedRing *r)
{
    const int slot = ring_oldest(r);
    if (slot < 0)
        return 0;
    ring_collected(r, slot);
    printf("collect %d\n", slot);
    return 1;
}

static FeedRing ring_of(int depth)
{
    FeedRing r;
    memset(&r, 0, sizeof(r));
    r.depth = depth;
    return r;
}

static void refused_run(const char *what, FeedRing *r, int ticks, int lag)
{
    int calls = 0;
    double ms = -1.0;
    last_error[0] = '\0';
    const int out = r  ?  ring_outstanding(r)  :  0;
    const int rc = ring_run(r, ticks, lag, &ms, [&] { calls++; return commit(r); }, [&] { calls++; return collect(r); });
    printf("refused run (%s): rc %d, \"%s\", calls %d, elapsed %s, outstanding %d -> %d\n", what, rc, last_error, calls,
           (ms == -1.0)  ?  "untouched"  :  "WRITTEN", out, r  ?  ring_outstanding(r)  :  0);
}

int main(void)
{
    for (int depth = 1;  depth <= kFeedMaxDepth;  depth++)
    {
        for (int lag = 1;  lag < depth;  lag++)
        {
            const int tick_counts[4] = {1, depth - 1, depth, 3*depth + 1};
            for (int ticks : tick_counts)
            {
                FeedRing r = ring_of(depth);
                double ms = -1.0;
                printf("run depth %d lag %d ticks %d\n", depth, lag, ticks);
                const int rc = ring_run(&r, ticks, lag, &ms, [&] { return commit(&r); }, [&] { return collect(&r); });
                printf("rc %d, outstanding %d, committed %lld, elapsed %s\n", rc, ring_outstanding(&r), r.n_commit, (ms >= 0.0)  ?  "written"  :  "MISSING");
            }
        }
    }
    printf("refusals\n");
    for (int depth = 0;  depth <= kFeedMaxDepth + 1;  depth++)
        printf("depth %d ok: %d\n", depth, (int) ring_depth_ok(depth));
    for (int depth = 1;  depth <= kFeedMaxDepth;  depth++)
    {
        FeedRing r = ring_of(depth);
        printf("depth %d\n", depth);
        printf("collect on an empty ring: oldest %d, outstanding %d\n", ring_oldest(&r), ring_outstanding(&r));
        refused_run("lag 0", &r, 1, 0);
        refused_run("lag = depth", &r, 1, depth);
        refused_run("no ticks", &r, 0, 1);
        FeedRing one = ring_of(depth);
        ring_committed(&one, ring_next(&one));
        refused_run("a tick outstanding", &one, 1, 1);
        printf("that tick: oldest %d, ", ring_oldest(&one));
        ring_collected(&one, ring_oldest(&one));
        printf("then oldest %d, outstanding %d\n", ring_oldest(&one), ring_outstanding(&one));
        // every slot busy: neither an acquire nor a commit gets a slot, and nothing moves
        while (ring_outstanding(&r) < depth)
            ring_committed(&r, ring_next(&r));
        last_error[0] = '\0';
        const int next = ring_next(&r);
        printf("every slot busy: next %d, \"%s\", ", next, last_error);
        printf("commit %d, outstanding %d, oldest %d\n", commit(&r), ring_outstanding(&r), ring_oldest(&r));
        // a commit that fails on tick k: the loop ends with its code, and the ring is where that tick found it
        for (int lag = 1;  lag < depth;  lag++)
        {
            for (int k = 0;  k <= depth;  k++)
            {
                FeedRing q = ring_of(depth);
                int tick = 0;
                int before = -1;
                double ms = -1.0;
                const int rc = ring_run(&q, depth + 1, lag, &ms,
                                        [&]
                                        {
                                            before = ring_outstanding(&q);
                                            return (tick++ == k)  ?  -77  :  (ring_committed(&q, ring_next(&q)), SPANGPU_OK);
                                        },
                                        [&] { ring_collected(&q, ring_oldest(&q)); return 0; });
                printf("lag %d, commit fails on tick %d: rc %d, outstanding %d -> %d, committed %lld, elapsed %s\n", lag, k, rc, before,
                       ring_outstanding(&q), q.n_commit, (ms == -1.0)  ?  "untouched"  :  "WRITTEN");
            }
        }
    }
    refused_run("no ring", nullptr, 1, 1);
    return 0;
}
