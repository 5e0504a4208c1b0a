/*
 * shim_group.h -- the staging protocol of every channel group behind include/spangpu_spandsp.h (tone, modem, line and echo
 * groups), written once.  Static functions, included by each shim: nothing here is exported, and nothing here touches a bank.
 *
 * N objects share one bank and one launch per tick.  An object stages one frame per tick; the tick runs when every attached
 * object has staged, or at the family's xxx_group_flush(); then the family replays the results per channel.  The threading
 * model: one mutex per group covers staging, attach / detach, the tick and every call on the bank; frames are copied in
 * outside it (a channel has one submitter, as a spandsp object has); the tick is synchronous and runs on the thread that
 * completes the set.  The mutex is recursive: a callback made during delivery may call back into its group.
 *
 * A family's group struct begins with a grp_core_t and supplies two hooks; the sample rows stay in the family's part.
 */
#ifndef SHIM_GROUP_H
#define SHIM_GROUP_H

#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct grp_core_s grp_core_t;

struct grp_core_s
{
    int n_ch;
    int max_samples;
    void **handles;             /* per channel: the attached state object or NULL */
    int32_t *lens;              /* per channel: samples staged for the tick being collected (0 = none) */
    int32_t *run;               /* ... and of the tick whose results are being delivered */
    int delivering;             /* a tick's callbacks are being made: staging from inside them waits for the next flush */
    int n_attached;
    int n_staged;
    pthread_mutex_t lock;
    /* Launch the tick over `lens` and fetch what the family replays (it may keep pointers in its part of the struct); < 0: failed */
    int (*run_tick)(grp_core_t *g);
    /* Replay the results for the channels with handles[c] && run[c] > 0 */
    void (*deliver)(grp_core_t *g);
};

/* The mutex is made even when an allocation fails, so that grp_free() is right after any grp_init(). */
static inline int grp_init(grp_core_t *g, int n_ch, int max_samples, int (*run_tick)(grp_core_t *), void (*deliver)(grp_core_t *))
{
    pthread_mutexattr_t at;

    g->n_ch = n_ch;
    g->max_samples = max_samples;
    g->run_tick = run_tick;
    g->deliver = deliver;
    g->handles = (void **) calloc(n_ch, sizeof(void *));
    g->lens = (int32_t *) calloc(n_ch, sizeof(int32_t));
    g->run = (int32_t *) calloc(n_ch, sizeof(int32_t));
    pthread_mutexattr_init(&at);
    pthread_mutexattr_settype(&at, PTHREAD_MUTEX_RECURSIVE);
    pthread_mutex_init(&g->lock, &at);
    pthread_mutexattr_destroy(&at);
    return (g->handles  &&  g->lens  &&  g->run)  ?  0  :  -1;
}

static inline void grp_free(grp_core_t *g)
{
    free(g->handles);
    free(g->lens);
    free(g->run);
    pthread_mutex_destroy(&g->lock);
}

/* Run the tick with the channels that have staged a frame.  The others sit it out -- untouched, as the reference's are when
   their xxx_rx() is not called -- and may stage for the next one.  Returns the number of channels that took part. */
static inline int grp_tick_locked(grp_core_t *g)
{
    int rc;
    int took;

    if (g->n_staged == 0)
        return 0;
    rc = g->run_tick(g);
    /* The tick is over, whatever came of it: its frames leave the staging area before anything is delivered -- a failure
       must not make every later call a "second frame" or run the same frames again, and a callback that stages a new
       frame finds a clean slate (that frame waits for the next tick). */
    took = g->n_staged;
    memcpy(g->run, g->lens, sizeof(int32_t)*g->n_ch);
    memset(g->lens, 0, sizeof(int32_t)*g->n_ch);
    g->n_staged = 0;
    if (rc < 0)
        return rc;
    g->delivering = 1;
    g->deliver(g);
    g->delivering = 0;
    return took;
}

/* The tick(s) that are due.  Callbacks may stage frames (a put_bit handler that answers by feeding its receiver, say): while
   a tick's callbacks run, a flush from inside them does nothing (`delivering`); when they are over, the tick those frames
   complete -- every attached channel has staged again -- runs at once instead of waiting for somebody to ask, so that no
   later xxx_rx() is refused as a second frame of a tick that nobody would ever have run. */
static inline int grp_flush_locked(grp_core_t *g)
{
    int total = 0;
    int rc;

    if (g->delivering)
        return 0;
    for (;;)
    {
        if ((rc = grp_tick_locked(g)) < 0)
            return rc;
        total += rc;
        if (g->n_staged == 0  ||  g->n_staged < g->n_attached)
            break;
    }
    return total;
}

static inline int grp_flush(grp_core_t *g)
{
    int rc;

    pthread_mutex_lock(&g->lock);
    rc = grp_flush_locked(g);
    pthread_mutex_unlock(&g->lock);
    return rc;
}

/* Is this thread inside one of the group's callbacks?  (Only the thread that delivers can see 1: it holds the lock.) */
static inline int grp_in_callback(grp_core_t *g)
{
    int rc;

    pthread_mutex_lock(&g->lock);
    rc = g->delivering;
    pthread_mutex_unlock(&g->lock);
    return rc;
}

/* Claim a slot for `handle`: tested and taken under the lock (two threads claiming one slot: one wins).  `fresh` (may be
   NULL) makes the channel a new object's before it is taken -- the slot may have served an earlier call; if it fails the
   slot stays free.  Returns 0, or -1. */
static inline int grp_claim(grp_core_t *g, int channel, void *handle, int (*fresh)(grp_core_t *g, int channel, void *arg), void *arg)
{
    int rc = -1;

    pthread_mutex_lock(&g->lock);
    if (g->handles[channel] == NULL  &&  (fresh == NULL  ||  fresh(g, channel, arg) >= 0))
    {
        g->handles[channel] = handle;
        g->n_attached++;
        rc = 0;
    }
    pthread_mutex_unlock(&g->lock);
    return rc;
}

/* Give a slot back.  Its frame of the tick being collected goes with it: nothing of it runs, nothing is delivered. */
static inline void grp_release(grp_core_t *g, int channel)
{
    pthread_mutex_lock(&g->lock);
    g->handles[channel] = NULL;
    g->n_attached--;
    if (g->lens[channel])
    {
        g->lens[channel] = 0;
        g->n_staged--;
    }
    if (g->n_staged > 0  &&  g->n_staged >= g->n_attached)
        grp_flush_locked(g);                /* it was the one the others were waiting for */
    pthread_mutex_unlock(&g->lock);
}

/* Stage one channel's frame (any thread) in two steps, the caller copying its rows in between, outside the lock:
   grp_stage_begin() refuses (-1) a second frame before the tick has run; grp_stage_commit() counts the frame and runs the
   tick if it was the last one awaited, returning what grp_flush_locked() does (0 if the tick is still being collected). */
static inline int grp_stage_begin(grp_core_t *g, int channel)
{
    int rc;

    pthread_mutex_lock(&g->lock);
    rc = (g->lens[channel])  ?  -1  :  0;
    pthread_mutex_unlock(&g->lock);
    return rc;
}

static inline int grp_stage_commit(grp_core_t *g, int channel, int samples)
{
    int rc;

    pthread_mutex_lock(&g->lock);
    g->lens[channel] = samples;
    g->n_staged++;
    rc = (g->n_staged >= g->n_attached)  ?  grp_flush_locked(g)  :  0;
    pthread_mutex_unlock(&g->lock);
    return rc;
}

/* A private object owns a one-channel group and takes whatever one call hands it: the buffer goes to channel 0 through the
   family's own staging function in pieces no longer than the staging row, each run at once.  Stops at the first piece for
   which `stage` returns < 0, and returns that. */
static inline int grp_feed_private(grp_core_t *g, const int16_t amp[], int samples,
                                   int (*stage)(grp_core_t *g, int channel, const int16_t amp[], int samples))
{
    int pos;
    int n;
    int rc;

    for (pos = 0;  pos < samples;  pos += n)
    {
        n = samples - pos;
        if (n > g->max_samples)
            n = g->max_samples;
        if ((rc = stage(g, 0, amp + pos, n)) < 0)
            return rc;
    }
    return 0;
}

#endif
