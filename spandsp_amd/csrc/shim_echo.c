/*
 * shim_echo.c -- host side (plain C) of the spandsp-named echo canceller entry points declared in
 * include/spangpu_spandsp.h (reference: src/spandsp/echo.h:145-185, src/echo.c:254-380,421-669).  An object made by
 * echo_can_init() is a private one-channel bank: echo_can_update() is then one kernel launch per SAMPLE -- the plumbing
 * configuration, there for source compatibility.  An object made by spangpu_echo_can_attach() is one channel of an echo
 * group's bank: its frames are staged, and the frames of all the group's objects run in one tick -- one launch per frame
 * length in the tick (spangpu_echo_update_var()).  No arithmetic of the canceller happens here.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

/* The threading model is the tone groups' (shim_tone.c): one mutex per group covers staging, attach / detach, the tick and
   every call on the bank; frames are copied in outside it (a channel has one submitter); the tick is synchronous and runs on
   the thread that completes the set. */
struct spangpu_echo_group_s
{
    spangpu_echo_t *bank;
    int n_ch;
    int taps;
    int max_samples;
    int16_t *stage_tx;          /* [n_ch][max_samples] */
    int16_t *stage_rx;
    int16_t *out_clean;         /* the tick's results, before they go to the buffers the callers named */
    int16_t *out_tx;
    echo_can_state_t **handles; /* per channel: the attached object or NULL */
    int32_t *lens;              /* per channel: samples staged for the tick being collected (0 = none) */
    uint8_t *hpf;               /* ... its use_hpf_tx */
    int16_t **clean_dst;        /* ... and where its results are to go */
    int16_t **tx_dst;
    int n_attached;
    int n_staged;
    int n_tx_dst;               /* staged frames that asked for tx_out */
    long long ticks;
    pthread_mutex_t lock;
};

struct echo_can_state_s
{
    spangpu_echo_t *bank;
    int taps;
    int16_t *snapshot;          /* tap set 0 as echo_can_snapshot() last saw it */
    spangpu_echo_group_t *grp;  /* NULL: a private one-channel bank */
    int channel;
};

/* Run the tick with the channels that have staged a frame; the others sit it out.  Returns the number of channels that
   took part.  The tick is over whatever came of it: a failure must not make every later frame a "second frame". */
static int echo_group_tick_locked(spangpu_echo_group_t *g)
{
    int rc;
    int c;

    if (g->n_staged == 0)
        return 0;
    rc = spangpu_echo_update_var(g->bank, g->stage_tx, g->stage_rx, g->out_clean, (g->n_tx_dst)  ?  g->out_tx  :  NULL,
                                 SPANGPU_MEM_HOST, g->lens, g->hpf, g->max_samples, g->max_samples);
    for (c = 0;  c < g->n_ch;  c++)
    {
        if (g->lens[c] == 0)
            continue;
        if (rc >= 0)
        {
            memcpy(g->clean_dst[c], g->out_clean + (size_t) c*g->max_samples, sizeof(int16_t)*g->lens[c]);
            if (g->tx_dst[c])
                memcpy(g->tx_dst[c], g->out_tx + (size_t) c*g->max_samples, sizeof(int16_t)*g->lens[c]);
        }
        g->lens[c] = 0;
        g->clean_dst[c] = NULL;
        g->tx_dst[c] = NULL;
    }
    g->n_staged = 0;
    g->n_tx_dst = 0;
    g->ticks++;
    return rc;
}

/* The object's channel is about to be read or changed: its staged frame, if it has one, runs first. */
static void echo_group_settle_locked(spangpu_echo_group_t *g, int channel)
{
    if (g->lens[channel])
        echo_group_tick_locked(g);
}

spangpu_echo_group_t *spangpu_echo_group_create(int device, int n_channels, int taps, int max_samples)
{
    spangpu_echo_group_t *g;
    size_t n;

    if (n_channels <= 0  ||  max_samples <= 0)
        return NULL;
    if ((g = (spangpu_echo_group_t *) calloc(1, sizeof(*g))) == NULL)
        return NULL;
    if (spangpu_echo_create(&g->bank, device, n_channels, taps, 0) != SPANGPU_OK)
    {
        free(g);
        return NULL;
    }
    g->n_ch = n_channels;
    g->taps = taps;
    g->max_samples = max_samples;
    n = (size_t) n_channels*max_samples;
    g->stage_tx = (int16_t *) calloc(n, sizeof(int16_t));
    g->stage_rx = (int16_t *) calloc(n, sizeof(int16_t));
    g->out_clean = (int16_t *) calloc(n, sizeof(int16_t));
    g->out_tx = (int16_t *) calloc(n, sizeof(int16_t));
    g->handles = (echo_can_state_t **) calloc(n_channels, sizeof(echo_can_state_t *));
    g->lens = (int32_t *) calloc(n_channels, sizeof(int32_t));
    g->hpf = (uint8_t *) calloc(n_channels, sizeof(uint8_t));
    g->clean_dst = (int16_t **) calloc(n_channels, sizeof(int16_t *));
    g->tx_dst = (int16_t **) calloc(n_channels, sizeof(int16_t *));
    pthread_mutex_init(&g->lock, NULL);
    if (g->stage_tx == NULL  ||  g->stage_rx == NULL  ||  g->out_clean == NULL  ||  g->out_tx == NULL  ||  g->handles == NULL
        ||  g->lens == NULL  ||  g->hpf == NULL  ||  g->clean_dst == NULL  ||  g->tx_dst == NULL)
    {
        spangpu_echo_group_destroy(g);
        return NULL;
    }
    return g;
}

/* (the objects attached to it are freed first: echo_can_free() reaches into its group) */
int spangpu_echo_group_destroy(spangpu_echo_group_t *g)
{
    if (g == NULL)
        return SPANGPU_OK;
    spangpu_echo_destroy(g->bank);
    free(g->stage_tx);
    free(g->stage_rx);
    free(g->out_clean);
    free(g->out_tx);
    free(g->handles);
    free(g->lens);
    free(g->hpf);
    free(g->clean_dst);
    free(g->tx_dst);
    pthread_mutex_destroy(&g->lock);
    free(g);
    return SPANGPU_OK;
}

int spangpu_echo_group_flush(spangpu_echo_group_t *g)
{
    int rc;

    if (g == NULL)
        return SPANGPU_ERR_BAD_ARG;
    pthread_mutex_lock(&g->lock);
    rc = echo_group_tick_locked(g);
    pthread_mutex_unlock(&g->lock);
    return rc;
}

long long spangpu_echo_group_ticks(const spangpu_echo_group_t *g)
{
    spangpu_echo_group_t *m = (spangpu_echo_group_t *) g;       /* (the lock is not part of what const promises) */
    long long n;

    if (g == NULL)
        return 0;
    pthread_mutex_lock(&m->lock);
    n = m->ticks;
    pthread_mutex_unlock(&m->lock);
    return n;
}

spangpu_echo_t *spangpu_echo_group_bank(spangpu_echo_group_t *g)
{
    return (g)  ?  g->bank  :  NULL;
}

echo_can_state_t *spangpu_echo_can_attach(spangpu_echo_group_t *g, int channel, int adaption_mode)
{
    echo_can_state_t *ec;

    if (g == NULL  ||  channel < 0  ||  channel >= g->n_ch)
        return NULL;
    if ((ec = (echo_can_state_t *) calloc(1, sizeof(*ec))) == NULL)
        return NULL;
    if ((ec->snapshot = (int16_t *) calloc((size_t) g->taps, sizeof(int16_t))) == NULL)
    {
        free(ec);
        return NULL;
    }
    ec->bank = g->bank;
    ec->taps = g->taps;
    ec->grp = g;
    ec->channel = channel;
    pthread_mutex_lock(&g->lock);
    if (g->handles[channel]  ||  spangpu_echo_reset_channel(g->bank, channel, adaption_mode) != SPANGPU_OK)
    {
        pthread_mutex_unlock(&g->lock);
        free(ec->snapshot);
        free(ec);
        return NULL;
    }
    g->handles[channel] = ec;
    g->n_attached++;
    pthread_mutex_unlock(&g->lock);
    return ec;
}

int spangpu_echo_can_pending(echo_can_state_t *ec)
{
    int rc;

    if (ec == NULL  ||  ec->grp == NULL)
        return 0;
    pthread_mutex_lock(&ec->grp->lock);
    rc = (ec->grp->lens[ec->channel] != 0);
    pthread_mutex_unlock(&ec->grp->lock);
    return rc;
}

static void echo_group_detach(echo_can_state_t *ec)
{
    spangpu_echo_group_t *g = ec->grp;
    int c = ec->channel;

    pthread_mutex_lock(&g->lock);
    if (g->handles[c] == ec)
    {
        g->handles[c] = NULL;
        g->n_attached--;
        if (g->lens[c])
        {
            /* a pending frame is dropped: nothing runs, nothing is written */
            if (g->tx_dst[c])
                g->n_tx_dst--;
            g->lens[c] = 0;
            g->clean_dst[c] = NULL;
            g->tx_dst[c] = NULL;
            g->n_staged--;
        }
        /* the channels that remain may all have been waiting for this one */
        if (g->n_staged > 0  &&  g->n_staged >= g->n_attached)
            echo_group_tick_locked(g);
    }
    pthread_mutex_unlock(&g->lock);
}

/* Stage one object's frame (any thread); the tick runs when every attached object has staged, or in
   spangpu_echo_group_flush().  The frame is copied outside the lock: a channel has one submitter, as a spandsp object has. */
static int echo_group_stage(echo_can_state_t *ec, const int16_t tx[], const int16_t rx[], int16_t clean[], int16_t tx_out[],
                            int n, int use_hpf_tx)
{
    spangpu_echo_group_t *g = ec->grp;
    int c = ec->channel;
    int rc;

    if (n > g->max_samples  ||  tx == NULL  ||  rx == NULL  ||  clean == NULL)
        return SPANGPU_ERR_BAD_ARG;
    pthread_mutex_lock(&g->lock);
    if (g->lens[c])
    {
        pthread_mutex_unlock(&g->lock);
        return SPANGPU_ERR_STATE;       /* second frame before the tick ran */
    }
    pthread_mutex_unlock(&g->lock);
    memcpy(g->stage_tx + (size_t) c*g->max_samples, tx, sizeof(int16_t)*n);
    memcpy(g->stage_rx + (size_t) c*g->max_samples, rx, sizeof(int16_t)*n);
    pthread_mutex_lock(&g->lock);
    g->lens[c] = n;
    g->hpf[c] = (use_hpf_tx)  ?  1  :  0;
    g->clean_dst[c] = clean;
    g->tx_dst[c] = tx_out;
    if (tx_out)
        g->n_tx_dst++;
    g->n_staged++;
    rc = SPANGPU_OK;
    if (g->n_staged >= g->n_attached)
    {
        rc = echo_group_tick_locked(g);
        if (rc > 0)
            rc = SPANGPU_OK;
    }
    pthread_mutex_unlock(&g->lock);
    return rc;
}

echo_can_state_t *echo_can_init(int len, int adaption_mode)
{
    echo_can_state_t *ec;

    if ((ec = (echo_can_state_t *) calloc(1, sizeof(*ec))) == NULL)
        return NULL;
    ec->taps = len;
    if ((ec->snapshot = (int16_t *) calloc((size_t) (len > 0  ?  len  :  1), sizeof(int16_t))) == NULL
        ||
        spangpu_echo_create(&ec->bank, 0, 1, len, adaption_mode) != SPANGPU_OK)
    {
        free(ec->snapshot);
        free(ec);
        return NULL;
    }
    return ec;
}

int echo_can_release(echo_can_state_t *ec)
{
    (void) ec;
    return 0;
}

int echo_can_free(echo_can_state_t *ec)
{
    if (ec)
    {
        if (ec->grp)
            echo_group_detach(ec);
        else
            spangpu_echo_destroy(ec->bank);
        free(ec->snapshot);
        free(ec);
    }
    return 0;
}

/* The calls below act on the object's channel: channel 0 of its own bank, or -- under the group's lock, after the frame it
   may have pending -- its channel of the group's. */
static void echo_enter(echo_can_state_t *ec)
{
    if (ec->grp)
    {
        pthread_mutex_lock(&ec->grp->lock);
        echo_group_settle_locked(ec->grp, ec->channel);
    }
}

static void echo_leave(echo_can_state_t *ec)
{
    if (ec->grp)
        pthread_mutex_unlock(&ec->grp->lock);
}

void echo_can_flush(echo_can_state_t *ec)
{
    echo_enter(ec);
    spangpu_echo_flush(ec->bank, ec->channel);
    echo_leave(ec);
}

void echo_can_adaption_mode(echo_can_state_t *ec, int adaption_mode)
{
    echo_enter(ec);
    spangpu_echo_adaption_mode(ec->bank, ec->channel, adaption_mode);
    echo_leave(ec);
}

/* src/echo.c:376-379: the working tap set (set 0) is copied aside.  The copy lives on the host: the four 16 bit sets of
   the one channel come back in one transfer and the first is kept. */
void echo_can_snapshot(echo_can_state_t *ec)
{
    int16_t *sets;

    if ((sets = (int16_t *) malloc((size_t) 4*ec->taps*sizeof(int16_t))) == NULL)
        return;
    echo_enter(ec);
    if (spangpu_echo_get_state(ec->bank, ec->channel, NULL, NULL, sets, NULL) == SPANGPU_OK)
        memcpy(ec->snapshot, sets, (size_t) ec->taps*sizeof(int16_t));
    echo_leave(ec);
    free(sets);
}

int spangpu_echo_can_snapshot_taps(echo_can_state_t *ec, int16_t *out, int max)
{
    int n;

    if (ec == NULL  ||  out == NULL  ||  max < 0)
        return -1;
    n = (max < ec->taps)  ?  max  :  ec->taps;
    echo_enter(ec);
    memcpy(out, ec->snapshot, (size_t) n*sizeof(int16_t));
    echo_leave(ec);
    return n;
}

int16_t echo_can_update(echo_can_state_t *ec, int16_t tx, int16_t rx)
{
    int16_t clean = 0;
    spangpu_echo_group_t *g = ec->grp;

    if (g)
    {
        /* whatever the group has staged runs first, then this one sample as a tick of one channel */
        size_t at = (size_t) ec->channel*g->max_samples;

        pthread_mutex_lock(&g->lock);
        echo_group_tick_locked(g);
        g->stage_tx[at] = tx;
        g->stage_rx[at] = rx;
        g->lens[ec->channel] = 1;
        g->hpf[ec->channel] = 0;
        if (spangpu_echo_update_var(g->bank, g->stage_tx, g->stage_rx, g->out_clean, NULL, SPANGPU_MEM_HOST, g->lens, g->hpf,
                                    g->max_samples, g->max_samples) == 1)
            clean = g->out_clean[at];
        g->lens[ec->channel] = 0;
        pthread_mutex_unlock(&g->lock);
        return clean;
    }
    spangpu_echo_update(ec->bank, &tx, &rx, &clean, SPANGPU_MEM_HOST, 1, 1, 0);
    return clean;
}

int16_t echo_can_hpf_tx(echo_can_state_t *ec, int16_t tx)
{
    int16_t out = tx;

    if (ec->grp)
    {
        pthread_mutex_lock(&ec->grp->lock);
        echo_group_tick_locked(ec->grp);
        spangpu_echo_hpf_tx_channel(ec->bank, ec->channel, &tx, &out, 1);
        pthread_mutex_unlock(&ec->grp->lock);
        return out;
    }
    spangpu_echo_hpf_tx(ec->bank, &tx, &out, 1, 1);
    return out;
}

/* n samples in one launch: clean[i] = echo_can_update(ec, use_hpf_tx ? echo_can_hpf_tx(ec, tx[i]) : tx[i], rx[i]);
   tx_out (may be NULL) receives the samples the canceller saw on the transmit side.  An attached object's frame is staged:
   clean and tx_out are filled when its group's tick has run (include/spangpu_spandsp.h). */
int spangpu_echo_can_update_block(echo_can_state_t *ec, const int16_t tx[], const int16_t rx[], int16_t clean[], int16_t tx_out[],
                                  int n, int use_hpf_tx)
{
    if (n <= 0)
        return 0;
    if (ec->grp)
        return echo_group_stage(ec, tx, rx, clean, tx_out, n, use_hpf_tx);
    return spangpu_echo_update_tx(ec->bank, tx, rx, clean, tx_out, SPANGPU_MEM_HOST, n, n, use_hpf_tx);
}

spangpu_echo_t *spangpu_echo_can_bank(echo_can_state_t *ec)
{
    if (ec == NULL)
        return NULL;
    echo_enter(ec);
    echo_leave(ec);
    return ec->bank;
}
