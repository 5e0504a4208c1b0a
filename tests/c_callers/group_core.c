/* The staging protocol of the channel groups (spandsp_amd/csrc/shim_group.h) on its own: no bank, no GPU.  A fake family --
 * one int16 row per channel, a run hook that records the lengths it was given, a deliver hook that records what it replays
 * and can stage frames from inside, as a callback would -- is driven through every rule of the protocol, then four threads
 * stage 50 ticks.  Built with -fsanitize=thread by tests/test_group_core.py.  Own code; exits 0 when every check held.
 *     group_core                                   (8 channels, rows of 16 samples, 4 threads) */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>

#include "shim_group.h"

#define N_CH    8
#define ROW     16
#define THREADS 4
#define TICKS   50

typedef struct
{
    grp_core_t core;
    int16_t rows[N_CH][ROW];
    int ticks;                      /* calls of the run hook */
    int delivers;                   /* calls of the deliver hook */
    int32_t seen[N_CH];             /* the lengths the run hook last saw */
    int32_t replayed[N_CH];         /* the lengths the deliver hook last replayed (0: channel not replayed) */
    int row_sum;                    /* the staged samples the run hook last saw, summed */
    int fail_next;                  /* the next run fails with this code */
    int restage;                    /* the next deliver stages a frame of `restage_len` for channels 0 .. restage - 1 */
    int restage_len;
    int inside;                     /* hooks running now */
    int reentered;                  /* a hook ran inside a hook */
    int full_ticks;                 /* runs in which every channel had a frame */
} fake_t;

static int failed;
static int ids[N_CH];

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "group_core: line %d: %s\n", __LINE__, #cond); failed = 1; } } while (0)

static int fake_stage(grp_core_t *g, int channel, const int16_t amp[], int samples)
{
    fake_t *f = (fake_t *) g;

    if (samples <= 0  ||  samples > g->max_samples)
        return -2;
    if (grp_stage_begin(g, channel) < 0)
        return -1;
    memcpy(f->rows[channel], amp, sizeof(int16_t)*samples);
    return grp_stage_commit(g, channel, samples);
}

/* a frame of `samples` samples, each of value `v` */
static int stage(fake_t *f, int channel, int samples, int v)
{
    int16_t amp[ROW];
    int i;

    for (i = 0;  i < ROW;  i++)
        amp[i] = (int16_t) v;
    return fake_stage(&f->core, channel, amp, samples);
}

static int fake_run(grp_core_t *g)
{
    fake_t *f = (fake_t *) g;
    int rc = f->fail_next;
    int full = 1;
    int c;
    int i;

    if (f->inside++)
        f->reentered = 1;
    f->ticks++;
    f->row_sum = 0;
    for (c = 0;  c < g->n_ch;  c++)
    {
        f->seen[c] = g->lens[c];
        for (i = 0;  i < g->lens[c];  i++)
            f->row_sum += f->rows[c][i];
        if (g->lens[c] == 0)
            full = 0;
    }
    f->full_ticks += full;
    f->fail_next = 0;
    f->inside--;
    return rc;
}

static void fake_deliver(grp_core_t *g)
{
    fake_t *f = (fake_t *) g;
    const int restage = f->restage;
    const int ticks = f->ticks;
    int c;

    if (f->inside++)
        f->reentered = 1;
    f->delivers++;
    f->restage = 0;
    for (c = 0;  c < g->n_ch;  c++)
        f->replayed[c] = (g->handles[c]  &&  g->run[c] > 0)  ?  g->run[c]  :  0;
    for (c = 0;  c < restage;  c++)
    {
        /* as a callback that feeds its receiver: accepted, and nothing runs before this delivery is over */
        CHECK(stage(f, c, f->restage_len, 1) == 0);
        CHECK(grp_flush(g) == 0);
        CHECK(grp_in_callback(g) == 1);
    }
    CHECK(f->ticks == ticks);
    f->inside--;
}

static int fresh_fails(grp_core_t *g, int channel, void *arg)
{
    (void) g;
    (void) channel;
    (void) arg;
    return -1;
}

static int fresh_counts(grp_core_t *g, int channel, void *arg)
{
    (void) g;
    (void) channel;
    ++*(int *) arg;
    return 0;
}

static void fake_new(fake_t *f, int n_ch, int n_claimed)
{
    int c;

    memset(f, 0, sizeof(*f));
    if (grp_init(&f->core, n_ch, ROW, fake_run, fake_deliver) < 0)
    {
        fprintf(stderr, "group_core: out of memory\n");
        exit(2);
    }
    for (c = 0;  c < n_claimed;  c++)
        CHECK(grp_claim(&f->core, c, &ids[c], NULL, NULL) == 0);
}

static int staged(const fake_t *f)
{
    int c;
    int n = 0;

    for (c = 0;  c < f->core.n_ch;  c++)
        n += (f->core.lens[c] != 0);
    return n;
}

/* The tick runs exactly when the last attached channel stages, with the staged lengths; a flush with channels missing runs
   the rest. */
static void test_tick_and_flush(void)
{
    fake_t f;
    int c;

    fake_new(&f, N_CH, N_CH);
    for (c = 0;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, c + 1, 2) == 0);
    CHECK(f.ticks == 0  &&  staged(&f) == N_CH - 1);
    CHECK(stage(&f, N_CH - 1, N_CH, 2) == N_CH);
    CHECK(f.ticks == 1  &&  f.delivers == 1  &&  staged(&f) == 0);
    CHECK(f.row_sum == 2*(N_CH*(N_CH + 1)/2));
    for (c = 0;  c < N_CH;  c++)
        CHECK(f.seen[c] == c + 1  &&  f.replayed[c] == c + 1);
    CHECK(grp_flush(&f.core) == 0  &&  f.ticks == 1);           /* nothing staged: no tick */
    for (c = 0;  c < 5;  c++)
        CHECK(stage(&f, c, ROW, 3) == 0);
    CHECK(grp_flush(&f.core) == 5  &&  f.ticks == 2);
    for (c = 0;  c < N_CH;  c++)
        CHECK(f.seen[c] == ((c < 5)  ?  ROW  :  0)  &&  f.replayed[c] == f.seen[c]);
    grp_free(&f.core);
}

/* A second frame before the tick is refused, and the first is intact. */
static void test_second_frame(void)
{
    fake_t f;

    fake_new(&f, N_CH, N_CH);
    CHECK(stage(&f, 0, 3, 5) == 0);
    CHECK(stage(&f, 0, 7, 9) == -1);
    CHECK(f.core.lens[0] == 3  &&  staged(&f) == 1);
    CHECK(grp_flush(&f.core) == 1);
    CHECK(f.seen[0] == 3  &&  f.row_sum == 3*5);
    grp_free(&f.core);
}

/* A failing run: the tick is over all the same, nothing is delivered, and the next frame of every channel is accepted. */
static void test_failed_run(void)
{
    fake_t f;
    int c;

    fake_new(&f, N_CH, N_CH);
    f.fail_next = -7;
    for (c = 0;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, 4, 1) == 0);
    CHECK(stage(&f, N_CH - 1, 4, 1) == -7);
    CHECK(f.ticks == 1  &&  f.delivers == 0  &&  staged(&f) == 0);
    for (c = 0;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, 6, 1) == 0);
    CHECK(stage(&f, N_CH - 1, 6, 1) == N_CH);
    CHECK(f.ticks == 2  &&  f.delivers == 1  &&  f.seen[0] == 6);
    f.fail_next = -7;
    CHECK(stage(&f, 2, 4, 1) == 0);
    CHECK(grp_flush(&f.core) == -7  &&  staged(&f) == 0);
    grp_free(&f.core);
}

/* Frames staged from inside deliver are never run re-entrantly.  If they complete the next set, that tick runs before the
   outer call returns; otherwise they wait. */
static void test_staging_from_inside(void)
{
    fake_t f;
    int c;

    fake_new(&f, N_CH, N_CH);
    f.restage = 1;                      /* channel 0 alone stages again: its frame waits */
    f.restage_len = 5;
    for (c = 0;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, 4, 1) == 0);
    CHECK(stage(&f, N_CH - 1, 4, 1) == N_CH);
    CHECK(f.ticks == 1  &&  staged(&f) == 1  &&  f.core.lens[0] == 5);
    CHECK(stage(&f, 0, 4, 1) == -1);
    for (c = 1;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, 4, 1) == 0);
    f.restage = N_CH;                   /* everybody stages again from inside: the tick after this one runs at once */
    f.restage_len = 9;
    CHECK(stage(&f, N_CH - 1, 4, 1) == 2*N_CH);
    CHECK(f.ticks == 3  &&  f.delivers == 3  &&  staged(&f) == 0);
    for (c = 0;  c < N_CH;  c++)
        CHECK(f.seen[c] == 9  &&  f.replayed[c] == 9);
    CHECK(!f.reentered);
    CHECK(grp_in_callback(&f.core) == 0);
    grp_free(&f.core);
}

/* Releasing the one channel the others were waiting for runs the tick; a released channel's pending frame is dropped. */
static void test_release(void)
{
    fake_t f;
    int c;

    fake_new(&f, N_CH, N_CH);
    for (c = 0;  c < N_CH - 1;  c++)
        CHECK(stage(&f, c, 4, 1) == 0);
    CHECK(f.ticks == 0);
    grp_release(&f.core, N_CH - 1);
    CHECK(f.ticks == 1  &&  f.seen[N_CH - 1] == 0  &&  f.seen[0] == 4  &&  staged(&f) == 0);
    CHECK(stage(&f, 0, 4, 1) == 0);
    CHECK(stage(&f, 1, 4, 1) == 0);
    grp_release(&f.core, 1);
    CHECK(f.ticks == 1  &&  staged(&f) == 1  &&  f.core.lens[1] == 0  &&  f.core.handles[1] == NULL);
    CHECK(grp_flush(&f.core) == 1);
    CHECK(f.ticks == 2  &&  f.seen[0] == 4  &&  f.seen[1] == 0  &&  f.replayed[1] == 0);
    /* the slot can be claimed again, and counts again */
    CHECK(grp_claim(&f.core, 1, &ids[1], NULL, NULL) == 0);
    for (c = 0;  c < N_CH - 2;  c++)
        CHECK(stage(&f, c, 4, 1) == 0);
    CHECK(f.ticks == 2);
    CHECK(stage(&f, N_CH - 2, 4, 1) == N_CH - 1);
    grp_free(&f.core);
}

/* A long buffer for a private object's one channel: pieces of at most a row, each run at once. */
static void test_private_feed(void)
{
    fake_t f;
    int16_t amp[2*ROW + 8];
    int i;

    fake_new(&f, 1, 1);
    for (i = 0;  i < 2*ROW + 8;  i++)
        amp[i] = (int16_t) i;
    CHECK(grp_feed_private(&f.core, amp, 2*ROW + 8, fake_stage) == 0);
    CHECK(f.ticks == 3  &&  f.seen[0] == 8  &&  f.row_sum == 8*2*ROW + 8*7/2);
    f.fail_next = -7;                   /* the first piece fails: the rest is not fed */
    CHECK(grp_feed_private(&f.core, amp, 2*ROW + 8, fake_stage) == -7);
    CHECK(f.ticks == 4  &&  staged(&f) == 0);
    grp_free(&f.core);
}

/* ---- threads ---- */
typedef struct
{
    fake_t *f;
    int index;
    pthread_barrier_t *gate;
    int claimed;
    int ok;
} worker_t;

static void *claimer(void *arg)
{
    worker_t *w = (worker_t *) arg;

    pthread_barrier_wait(w->gate);
    w->claimed = (grp_claim(&w->f->core, 3, &ids[w->index], NULL, NULL) == 0);
    return NULL;
}

/* Two threads claim one slot: exactly one wins.  A slot whose `fresh` hook fails stays free. */
static void test_claim(void)
{
    fake_t f;
    pthread_barrier_t gate;
    pthread_t th[2];
    worker_t w[2];
    int freshened = 0;
    int i;

    fake_new(&f, N_CH, 0);
    CHECK(grp_claim(&f.core, 3, &ids[0], fresh_fails, NULL) == -1);
    CHECK(f.core.handles[3] == NULL);
    pthread_barrier_init(&gate, NULL, 2);
    for (i = 0;  i < 2;  i++)
    {
        w[i].f = &f;
        w[i].index = i;
        w[i].gate = &gate;
        w[i].claimed = 0;
        pthread_create(&th[i], NULL, claimer, &w[i]);
    }
    for (i = 0;  i < 2;  i++)
        pthread_join(th[i], NULL);
    pthread_barrier_destroy(&gate);
    CHECK(w[0].claimed + w[1].claimed == 1);
    CHECK(f.core.handles[3] == &ids[(w[0].claimed)  ?  0  :  1]);
    CHECK(grp_claim(&f.core, 3, &ids[2], fresh_counts, &freshened) == -1  &&  freshened == 0);     /* taken: not touched */
    CHECK(grp_claim(&f.core, 4, &ids[4], fresh_counts, &freshened) == 0  &&  freshened == 1);
    /* one tick of the two claimed channels: the slot was counted once */
    CHECK(stage(&f, 3, 4, 1) == 0);
    CHECK(stage(&f, 4, 4, 1) == 2);
    grp_free(&f.core);
}

static void *stager(void *arg)
{
    worker_t *w = (worker_t *) arg;
    const int per = N_CH/THREADS;
    int t;
    int c;

    for (t = 0;  t < TICKS;  t++)
    {
        for (c = w->index*per;  c < (w->index + 1)*per;  c++)
        {
            if (stage(w->f, c, 1 + (t + c)%ROW, 1) < 0)
                w->ok = 0;
        }
        /* everybody has staged, so the tick has run: on the thread that completed the set */
        pthread_barrier_wait(w->gate);
    }
    return NULL;
}

/* Four threads, two channels each, 50 ticks: every tick saw all the channels. */
static void test_threads(void)
{
    fake_t f;
    pthread_barrier_t gate;
    pthread_t th[THREADS];
    worker_t w[THREADS];
    int i;

    fake_new(&f, N_CH, N_CH);
    pthread_barrier_init(&gate, NULL, THREADS);
    for (i = 0;  i < THREADS;  i++)
    {
        w[i].f = &f;
        w[i].index = i;
        w[i].gate = &gate;
        w[i].ok = 1;
        pthread_create(&th[i], NULL, stager, &w[i]);
    }
    for (i = 0;  i < THREADS;  i++)
    {
        pthread_join(th[i], NULL);
        CHECK(w[i].ok);
    }
    pthread_barrier_destroy(&gate);
    CHECK(f.ticks == TICKS  &&  f.full_ticks == TICKS  &&  f.delivers == TICKS  &&  staged(&f) == 0);
    for (i = 0;  i < N_CH;  i++)
        CHECK(f.seen[i] == 1 + (TICKS - 1 + i)%ROW  &&  f.replayed[i] == f.seen[i]);
    grp_free(&f.core);
}

int main(void)
{
    test_tick_and_flush();
    test_second_frame();
    test_failed_run();
    test_staging_from_inside();
    test_release();
    test_private_feed();
    test_claim();
    test_threads();
    if (!failed)
        printf("group_core: %d channels, %d threads, %d ticks: ok\n", N_CH, THREADS, TICKS);
    return failed;
}
