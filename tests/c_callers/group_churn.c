/*
 * group_churn.c -- slot churn on a shared group at bank scale, through the spandsp-named entry points alone.
 *
 *   group_churn churn <input> <output>     DTMF or V.29 9600 group driven by T worker threads
 *   group_churn race <v29|fsk|mct> <n>     n fresh two-slot groups, four threads attaching the same free slot at once
 *
 * churn: the input holds R base signals and a schedule of one byte per class and tick; channel c plays base c % R on
 * schedule c % R.  Each worker owns a contiguous slice of channels and per tick stages, sits out, changes a per-object
 * setting, or frees its object and attaches a new one (a new call) before staging.  Ticks in which every channel stages
 * run from inside the last xxx_rx(); the others are run by worker 0's flush.  Every channel keeps an event count and a
 * running hash of (call, event); channels named in the input also keep the full log.  The output holds those, the
 * count of unexpected xxx_rx() results per channel, and the wall time of every tick.
 */
#define _POSIX_C_SOURCE 200112L
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "spangpu_spandsp.h"

#define FRAME       160
#define SHORT       80

enum { S_STAGE = 0, S_SHORT = 1, S_SKIP = 2, S_SETTING = 3, S_NEW_CALL = 4, S_SECOND = 5 };
enum { K_DTMF = 0, K_V29 = 1 };

typedef struct
{
    uint32_t count;
    uint32_t errors;
    uint64_t hash;
    int32_t call;
    int32_t pos;
    int logged;
    int n_log;
    int cap_log;
    int32_t *log;
    void *obj;
} chan_t;

static int kind;
static int n_ch;
static int ticks;
static int n_classes;
static int n_threads;
static uint8_t *sched;
static int16_t *bases;
static chan_t *ch;
static spangpu_group_t *tgrp;
static spangpu_modem_group_t *mgrp;
static pthread_barrier_t bar;
static double *tick_ms;

static double now_ms(void)
{
    struct timespec t;

    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec*1.0e3 + t.tv_nsec*1.0e-6;
}

static void event(chan_t *s, int v)
{
    uint32_t w[2];
    const uint8_t *b = (const uint8_t *) w;
    int i;

    w[0] = (uint32_t) s->call;
    w[1] = (uint32_t) v;
    for (i = 0;  i < 8;  i++)
        s->hash = (s->hash ^ b[i])*UINT64_C(1099511628211);
    s->count++;
    if (s->logged)
    {
        if (s->n_log + 2 > s->cap_log)
        {
            s->cap_log = (s->cap_log)  ?  2*s->cap_log  :  4096;
            if ((s->log = (int32_t *) realloc(s->log, s->cap_log*sizeof(int32_t))) == NULL)
                abort();
        }
        s->log[s->n_log++] = s->call;
        s->log[s->n_log++] = v;
    }
}

static void on_digits(void *user, const char *digits, int len)
{
    int i;

    for (i = 0;  i < len;  i++)
        event((chan_t *) user, (unsigned char) digits[i]);
}

static void on_bit(void *user, int bit)
{
    event((chan_t *) user, bit);
}

static void *attach(int c)
{
    if (kind == K_DTMF)
        return spangpu_dtmf_rx_attach(tgrp, c, on_digits, &ch[c]);
    return spangpu_v29_rx_attach(mgrp, c, on_bit, &ch[c]);
}

static void release(int c)
{
    if (kind == K_DTMF)
        dtmf_rx_free((dtmf_rx_state_t *) ch[c].obj);
    else
        v29_rx_free((v29_rx_state_t *) ch[c].obj);
    ch[c].obj = NULL;
}

static int rx(int c, const int16_t *amp, int len)
{
    if (kind == K_DTMF)
        return dtmf_rx((dtmf_rx_state_t *) ch[c].obj, amp, len);
    return v29_rx((v29_rx_state_t *) ch[c].obj, amp, len);
}

static void step(int c, int k)
{
    chan_t *s = &ch[c];
    const int cls = c % n_classes;
    const int code = sched[(size_t) cls*ticks + k];
    const int16_t *base = bases + (size_t) cls*ticks*FRAME;
    int len = (code == S_SHORT)  ?  SHORT  :  FRAME;

    if (code == S_SKIP)
        return;
    if (code == S_NEW_CALL)
    {
        release(c);
        s->call++;
        if ((s->obj = attach(c)) == NULL)
        {
            s->errors++;
            return;
        }
    }
    if (code == S_SETTING)
    {
        if (kind == K_DTMF)
            dtmf_rx_parms((dtmf_rx_state_t *) s->obj, -1, 6.0f, 6.0f, -36.0f);
        else
            v29_rx_set_signal_cutoff((v29_rx_state_t *) s->obj, -40.0f);
    }
    if (rx(c, base + s->pos, len) != 0)
        s->errors++;
    if (code == S_SECOND  &&  rx(c, base + s->pos, len) != -1)
        s->errors++;                    /* a second frame before the tick has run is refused */
    s->pos += len;
}

static void *worker(void *arg)
{
    const int t = (int) (intptr_t) arg;
    const int lo = (int) ((long long) n_ch*t/n_threads);
    const int hi = (int) ((long long) n_ch*(t + 1)/n_threads);
    double t0 = 0.0;
    int k;
    int c;

    for (k = 0;  k < ticks;  k++)
    {
        pthread_barrier_wait(&bar);
        if (t == 0)
            t0 = now_ms();
        for (c = lo;  c < hi;  c++)
            step(c, k);
        pthread_barrier_wait(&bar);
        if (t == 0)
        {
            if (kind == K_DTMF)
                spangpu_group_flush(tgrp);
            else
                spangpu_modem_group_flush(mgrp);
            tick_ms[k] = now_ms() - t0;
        }
    }
    return NULL;
}

static int read_all(FILE *f, void *p, size_t n)
{
    return fread(p, 1, n, f) == n;
}

static int churn(const char *in, const char *out)
{
    FILE *f;
    int32_t hdr[6];
    int32_t *logged = NULL;
    pthread_t *th;
    int c;
    int k;
    int t;

    if ((f = fopen(in, "rb")) == NULL  ||  !read_all(f, hdr, sizeof(hdr)))
        return 2;
    kind = hdr[0];
    n_ch = hdr[1];
    ticks = hdr[2];
    n_classes = hdr[3];
    n_threads = hdr[4];
    sched = (uint8_t *) malloc((size_t) n_classes*ticks);
    bases = (int16_t *) malloc((size_t) n_classes*ticks*FRAME*sizeof(int16_t));
    logged = (int32_t *) malloc((size_t) (hdr[5] + 1)*sizeof(int32_t));
    ch = (chan_t *) calloc(n_ch, sizeof(chan_t));
    tick_ms = (double *) calloc(ticks, sizeof(double));
    th = (pthread_t *) calloc(n_threads, sizeof(pthread_t));
    if (sched == NULL  ||  bases == NULL  ||  logged == NULL  ||  ch == NULL  ||  tick_ms == NULL  ||  th == NULL
        ||  !read_all(f, sched, (size_t) n_classes*ticks)
        ||  !read_all(f, bases, (size_t) n_classes*ticks*FRAME*sizeof(int16_t))
        ||  !read_all(f, logged, (size_t) hdr[5]*sizeof(int32_t)))
        return 2;
    fclose(f);
    for (k = 0;  k < hdr[5];  k++)
        ch[logged[k]].logged = 1;
    for (c = 0;  c < n_ch;  c++)
        ch[c].hash = UINT64_C(14695981039346656037);
    if (kind == K_DTMF)
        tgrp = spangpu_group_create(0, SPANGPU_DTMF, n_ch, FRAME, NULL);
    else
        mgrp = spangpu_modem_group_create(0, SPANGPU_V29, n_ch, 9600, FRAME);
    if (tgrp == NULL  &&  mgrp == NULL)
        return 3;
    for (c = 0;  c < n_ch;  c++)
    {
        if ((ch[c].obj = attach(c)) == NULL)
            return 3;
    }
    pthread_barrier_init(&bar, NULL, n_threads);
    for (t = 0;  t < n_threads;  t++)
        pthread_create(&th[t], NULL, worker, (void *) (intptr_t) t);
    for (t = 0;  t < n_threads;  t++)
        pthread_join(th[t], NULL);
    pthread_barrier_destroy(&bar);
    for (c = 0;  c < n_ch;  c++)
        release(c);
    if (kind == K_DTMF)
        spangpu_group_destroy(tgrp);
    else
        spangpu_modem_group_destroy(mgrp);

    if ((f = fopen(out, "wb")) == NULL)
        return 2;
    for (c = 0;  c < n_ch;  c++)
    {
        fwrite(&ch[c].count, 4, 1, f);
        fwrite(&ch[c].errors, 4, 1, f);
        fwrite(&ch[c].hash, 8, 1, f);
    }
    fwrite(tick_ms, sizeof(double), ticks, f);
    for (k = 0;  k < hdr[5];  k++)
    {
        c = logged[k];
        fwrite(&c, 4, 1, f);
        fwrite(&ch[c].n_log, 4, 1, f);
        fwrite(ch[c].log, 4, ch[c].n_log, f);
    }
    fclose(f);
    {
        double sum = 0.0;

        for (k = 0;  k < ticks;  k++)
            sum += tick_ms[k];
        printf("group_churn %s: %d channels, %d ticks, %d threads, mean tick %.3f ms\n", (kind == K_DTMF)  ?  "dtmf"  :  "v29",
               n_ch, ticks, n_threads, sum/ticks);
    }
    return 0;
}

/* ---- race: several threads attach the same free slot at the same moment -------------------------------------------- */
static volatile int go;
static volatile int ready;
static pthread_mutex_t ready_lock = PTHREAD_MUTEX_INITIALIZER;
static const char *race_kind;
static spangpu_line_group_t *lgrp;
static void *won[4];

static void on_tone(void *user, int code, int level, int delay)
{
    (void) user;
    (void) code;
    (void) level;
    (void) delay;
}

static void *race_attach(int channel)
{
    if (strcmp(race_kind, "v29") == 0)
        return spangpu_v29_rx_attach(mgrp, channel, on_bit, NULL);
    if (strcmp(race_kind, "fsk") == 0)
        return spangpu_fsk_rx_attach(lgrp, channel, on_bit, NULL);
    return spangpu_modem_connect_tones_rx_attach(lgrp, channel, on_tone, NULL);
}

static int race_rx(void *obj, const int16_t *amp)
{
    if (strcmp(race_kind, "v29") == 0)
        return v29_rx((v29_rx_state_t *) obj, amp, FRAME);
    if (strcmp(race_kind, "fsk") == 0)
        return fsk_rx((fsk_rx_state_t *) obj, amp, FRAME);
    return modem_connect_tones_rx((modem_connect_tones_rx_state_t *) obj, amp, FRAME);
}

static void race_free(void *obj)
{
    if (strcmp(race_kind, "v29") == 0)
        v29_rx_free((v29_rx_state_t *) obj);
    else if (strcmp(race_kind, "fsk") == 0)
        fsk_rx_free((fsk_rx_state_t *) obj);
    else
        modem_connect_tones_rx_free((modem_connect_tones_rx_state_t *) obj);
}

static void *racer(void *arg)
{
    const int i = (int) (intptr_t) arg;

    pthread_mutex_lock(&ready_lock);
    ready++;
    pthread_mutex_unlock(&ready_lock);
    while (!go)
        ;
    won[i] = race_attach(0);
    return NULL;
}

static int race(const char *what, int rounds)
{
    static const int16_t silence[FRAME];
    pthread_t th[4];
    int r;
    int i;
    int n_won;
    int bad = 0;

    race_kind = what;
    for (r = 0;  r < rounds;  r++)
    {
        void *other;
        void *winner = NULL;

        mgrp = NULL;
        lgrp = NULL;
        if (strcmp(what, "v29") == 0)
            mgrp = spangpu_modem_group_create(0, SPANGPU_V29, 2, 9600, FRAME);
        else if (strcmp(what, "fsk") == 0)
            lgrp = spangpu_fsk_group_create(0, &preset_fsk_specs[FSK_V21CH2], FSK_FRAME_MODE_SYNC, 2, FRAME);
        else
            lgrp = spangpu_modem_connect_tones_group_create(0, MODEM_CONNECT_TONES_ANS, 1, 2, FRAME);
        if ((mgrp == NULL  &&  lgrp == NULL)  ||  (other = race_attach(1)) == NULL)
            return 3;
        go = 0;
        ready = 0;
        for (i = 0;  i < 4;  i++)
            pthread_create(&th[i], NULL, racer, (void *) (intptr_t) i);
        for (;;)
        {
            pthread_mutex_lock(&ready_lock);
            i = ready;
            pthread_mutex_unlock(&ready_lock);
            if (i == 4)
                break;
        }
        go = 1;
        for (i = 0;  i < 4;  i++)
            pthread_join(th[i], NULL);
        for (i = 0, n_won = 0;  i < 4;  i++)
        {
            if (won[i])
            {
                n_won++;
                winner = won[i];
            }
        }
        if (n_won != 1)
            bad++;
        /* both slots stage: the tick runs by itself, so a second round of frames is accepted */
        for (i = 0;  i < 2  &&  winner;  i++)
        {
            if (race_rx(winner, silence) != 0  ||  race_rx(other, silence) != 0)
            {
                bad++;
                break;
            }
        }
        for (i = 0;  i < 4;  i++)
        {
            if (won[i])
                race_free(won[i]);
        }
        race_free(other);
        if (mgrp)
            spangpu_modem_group_destroy(mgrp);
        if (lgrp)
            spangpu_line_group_destroy(lgrp);
    }
    printf("group_churn race %s: %d rounds, %d bad\n", what, rounds, bad);
    return bad  ?  1  :  0;
}

int main(int argc, char *argv[])
{
    if (argc == 4  &&  strcmp(argv[1], "churn") == 0)
        return churn(argv[2], argv[3]);
    if (argc == 4  &&  strcmp(argv[1], "race") == 0)
        return race(argv[2], atoi(argv[3]));
    fprintf(stderr, "usage: group_churn churn <input> <output> | group_churn race <v29|fsk|mct> <rounds>\n");
    return 2;
}
