/* A C caller of the echo canceller groups: N echo_can_state_t objects attached to one group, their 160-sample frames staged
 * by T threads -- every thread owns its own objects -- through spangpu_echo_can_update_block(); the tick runs on whichever
 * thread completes the set.  A second pass stages the same lines from one thread into a fresh group: the CRC-32 of all clean
 * samples must be the same.  The time from the first frame staged to the tick run is reported per tick (the lines are made
 * before the clock starts).  Own code; exits 0 on success, non-zero on any mismatch or error code.
 *     echo_group [objects [threads [ticks]]]       (defaults 1024 16 50) */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "spangpu_spandsp.h"

#define FRAME 160
#define TAPS 128

typedef struct
{
    unsigned lcg;
    int hist[4];
} line_t;

typedef struct run_s
{
    int n_obj;
    int n_threads;
    int ticks;
    spangpu_echo_group_t *grp;
    echo_can_state_t **ec;
    line_t *line;
    int16_t *tx;                    /* [n_obj][FRAME]: the tick's frames */
    int16_t *rx;
    int16_t *clean;
    double ms;                      /* staging + tick, summed over the ticks */
    pthread_barrier_t ready;        /* every thread has made its objects' frames */
    pthread_barrier_t staged;       /* every thread has staged its objects' frames: the tick has run */
    pthread_barrier_t summed;       /* ... and its samples are in the CRC */
    unsigned long crc;
    double e_rx;
    double e_clean;
    int failed;
} run_t;

typedef struct
{
    run_t *run;
    int index;
} worker_t;

static unsigned long crc_table[256];

static void crc_init(void)
{
    unsigned long c;
    int n;
    int k;

    for (n = 0;  n < 256;  n++)
    {
        c = (unsigned long) n;
        for (k = 0;  k < 8;  k++)
            c = (c & 1)  ?  (0xEDB88320UL ^ (c >> 1))  :  (c >> 1);
        crc_table[n] = c;
    }
}

static unsigned long crc_add(unsigned long crc, const int16_t *s, int n)
{
    int i;

    for (i = 0;  i < n;  i++)
    {
        crc = crc_table[(crc ^ (unsigned long) (s[i] & 0xFF)) & 0xFF] ^ (crc >> 8);
        crc = crc_table[(crc ^ (unsigned long) ((s[i] >> 8) & 0xFF)) & 0xFF] ^ (crc >> 8);
    }
    return crc;
}

/* white noise out, an echo through a four-tap path back: the line of object c is a function of c alone */
static void next_frame(line_t *ln, int c, int16_t tx[], int16_t rx[])
{
    int i;
    int k;
    int acc;

    for (i = 0;  i < FRAME;  i++)
    {
        acc = 0;
        for (k = 0;  k < 4;  k++)
        {
            ln->lcg = ln->lcg*1664525u + 1013904223u;
            acc += (int) ((ln->lcg >> 16) & 0x3FFF) - 0x2000;
        }
        tx[i] = (int16_t) (acc/4);
        ln->hist[3] = ln->hist[2];
        ln->hist[2] = ln->hist[1];
        ln->hist[1] = ln->hist[0];
        ln->hist[0] = tx[i];
        rx[i] = (int16_t) ((ln->hist[1]*(40 + c%50) - ln->hist[2]*60 + ln->hist[3]*25)/256);
    }
}

static void *worker(void *arg)
{
    worker_t *w = (worker_t *) arg;
    run_t *r = w->run;
    int per = (r->n_obj + r->n_threads - 1)/r->n_threads;
    int lo = w->index*per;
    int hi = (lo + per < r->n_obj)  ?  (lo + per)  :  r->n_obj;
    struct timespec t0;
    struct timespec t1;
    int16_t *tx;
    int16_t *rx;
    int t;
    int c;
    int i;

    for (t = 0;  t < r->ticks;  t++)
    {
        for (c = lo;  c < hi;  c++)
            next_frame(&r->line[c], c, r->tx + (size_t) c*FRAME, r->rx + (size_t) c*FRAME);
        pthread_barrier_wait(&r->ready);
        if (w->index == 0)
            clock_gettime(CLOCK_MONOTONIC, &t0);
        for (c = lo;  c < hi;  c++)
        {
            tx = r->tx + (size_t) c*FRAME;
            rx = r->rx + (size_t) c*FRAME;
            if (spangpu_echo_can_update_block(r->ec[c], tx, rx, r->clean + (size_t) c*FRAME, NULL, FRAME, 0) != SPANGPU_OK)
            {
                fprintf(stderr, "object %d, tick %d: staging failed: %s\n", c, t, spangpu_last_error());
                r->failed = 1;
            }
            if (w->index == 0  &&  c == lo  &&  t >= r->ticks - 10)
            {
                for (i = 0;  i < FRAME;  i++)
                    r->e_rx += (double) rx[i]*rx[i];
            }
        }
        pthread_barrier_wait(&r->staged);
        if (w->index == 0)
        {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            r->ms += 1.0e3*(double) (t1.tv_sec - t0.tv_sec) + 1.0e-6*(double) (t1.tv_nsec - t0.tv_nsec);
        }
        for (c = lo;  c < hi;  c++)
        {
            if (spangpu_echo_can_pending(r->ec[c]))
            {
                fprintf(stderr, "object %d, tick %d: still pending after the set was complete\n", c, t);
                r->failed = 1;
            }
        }
        if (w->index == 0)
        {
            if (spangpu_echo_group_ticks(r->grp) != t + 1)
            {
                fprintf(stderr, "tick %d: the group has run %lld ticks\n", t, spangpu_echo_group_ticks(r->grp));
                r->failed = 1;
            }
            r->crc = crc_add(r->crc, r->clean, r->n_obj*FRAME);
            if (t >= r->ticks - 10)
            {
                for (i = 0;  i < FRAME;  i++)
                    r->e_clean += (double) r->clean[i]*r->clean[i];
            }
        }
        pthread_barrier_wait(&r->summed);
    }
    return NULL;
}

/* One pass: a fresh group, n_obj objects, staged from n_threads threads.  Returns the CRC-32 of every clean sample, in
   (tick, object, sample) order; *failed is set on any error. */
static unsigned long pass(int n_obj, int n_threads, int ticks, int *failed, double *ms_per_tick)
{
    run_t r;
    pthread_t *th;
    worker_t *wk;
    int c;
    int i;

    memset(&r, 0, sizeof(r));
    r.n_obj = n_obj;
    r.n_threads = n_threads;
    r.ticks = ticks;
    r.crc = 0xFFFFFFFFUL;
    r.ec = (echo_can_state_t **) calloc((size_t) n_obj, sizeof(echo_can_state_t *));
    r.line = (line_t *) calloc((size_t) n_obj, sizeof(line_t));
    r.clean = (int16_t *) calloc((size_t) n_obj*FRAME, sizeof(int16_t));
    r.tx = (int16_t *) calloc((size_t) n_obj*FRAME, sizeof(int16_t));
    r.rx = (int16_t *) calloc((size_t) n_obj*FRAME, sizeof(int16_t));
    th = (pthread_t *) calloc((size_t) n_threads, sizeof(pthread_t));
    wk = (worker_t *) calloc((size_t) n_threads, sizeof(worker_t));
    if (r.ec == NULL  ||  r.line == NULL  ||  r.clean == NULL  ||  r.tx == NULL  ||  r.rx == NULL  ||  th == NULL  ||  wk == NULL)
    {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    if ((r.grp = spangpu_echo_group_create(0, n_obj, TAPS, FRAME)) == NULL)
    {
        fprintf(stderr, "spangpu_echo_group_create failed: %s\n", spangpu_last_error());
        exit(2);
    }
    for (c = 0;  c < n_obj;  c++)
    {
        r.line[c].lcg = 12345u + 7919u*(unsigned) c;
        if ((r.ec[c] = spangpu_echo_can_attach(r.grp, c, ECHO_CAN_USE_ADAPTION)) == NULL)
        {
            fprintf(stderr, "attach %d failed: %s\n", c, spangpu_last_error());
            exit(2);
        }
    }
    pthread_barrier_init(&r.ready, NULL, (unsigned) n_threads);
    pthread_barrier_init(&r.staged, NULL, (unsigned) n_threads);
    pthread_barrier_init(&r.summed, NULL, (unsigned) n_threads);
    for (i = 0;  i < n_threads;  i++)
    {
        wk[i].run = &r;
        wk[i].index = i;
        if (pthread_create(&th[i], NULL, worker, &wk[i]) != 0)
        {
            fprintf(stderr, "pthread_create failed\n");
            exit(2);
        }
    }
    for (i = 0;  i < n_threads;  i++)
        pthread_join(th[i], NULL);
    pthread_barrier_destroy(&r.ready);
    pthread_barrier_destroy(&r.staged);
    pthread_barrier_destroy(&r.summed);
    if (spangpu_echo_group_flush(r.grp) != 0)
    {
        fprintf(stderr, "frames were left over\n");
        r.failed = 1;
    }
    for (c = 0;  c < n_obj;  c++)
        echo_can_free(r.ec[c]);
    spangpu_echo_group_destroy(r.grp);
    /* the canceller of object 0 has done something to its line */
    if (!(r.e_clean < r.e_rx))
    {
        fprintf(stderr, "object 0: residue %g against %g received\n", r.e_clean, r.e_rx);
        r.failed = 1;
    }
    free(r.ec);
    free(r.line);
    free(r.clean);
    free(r.tx);
    free(r.rx);
    free(th);
    free(wk);
    if (r.failed)
        *failed = 1;
    *ms_per_tick = r.ms/ticks;
    return r.crc ^ 0xFFFFFFFFUL;
}

int main(int argc, char *argv[])
{
    int n_obj = (argc > 1)  ?  atoi(argv[1])  :  1024;
    int n_threads = (argc > 2)  ?  atoi(argv[2])  :  16;
    int ticks = (argc > 3)  ?  atoi(argv[3])  :  50;
    int failed = 0;
    unsigned long many;
    unsigned long one;
    double ms_many = 0.0;
    double ms_one = 0.0;

    if (n_obj < 1  ||  n_threads < 1  ||  n_threads > n_obj  ||  ticks < 10)
    {
        fprintf(stderr, "usage: echo_group [objects [threads [ticks >= 10]]]\n");
        return 2;
    }
    crc_init();
    many = pass(n_obj, n_threads, ticks, &failed, &ms_many);
    one = pass(n_obj, 1, ticks, &failed, &ms_one);
    printf("echo_group: %d objects, %d ticks: CRC-32 %08lx from %d threads, %08lx from one\n", n_obj, ticks, many, n_threads, one);
    printf("echo_group: staging and tick, ms per tick: %.3f from %d threads, %.3f from one\n", ms_many, n_threads, ms_one);
    return (failed  ||  many != one)  ?  1  :  0;
}
