/*
 * shim_echo.c -- host side (plain C) of the spandsp-named echo canceller entry points declared in
 * include/spangpu_spandsp.h (reference: src/spandsp/echo.h:145-185, src/echo.c:254-380,421-669).  An object made by
 * echo_can_init() is a private one-channel bank: echo_can_update() is then one kernel launch per SAMPLE -- the plumbing
 * configuration, there for source compatibility.  An object made by spangpu_echo_can_attach() is one channel of an echo
 * group's bank: its frames are staged, and the frames of all the group's objects run in one tick -- one launch per frame
 * length in the tick (spangpu_echo_update_var()).  No arithmetic of the canceller happens here.
 */
#include "spangpu_spandsp.h"
#include "shim_group.h"

/* The staging protocol and its threading model are every group's: shim_group.h.  This family's delivery makes no callbacks
   -- it copies the results to the buffers the callers named -- so nothing re-enters a tick here. */
struct spangpu_echo_group_s
{
    grp_core_t core;
    spangpu_echo_t *bank;
    int taps;
    int16_t *stage_tx;          /* [n_ch][max_samples] */
    int16_t *stage_rx;
    int16_t *out_clean;         /* the tick's results, before they go to the buffers the callers named */
    int16_t *out_tx;
    uint8_t *hpf;               /* per channel: the staged frame's use_hpf_tx */
    int16_t **clean_dst;        /* ... and where its results are to go */
    int16_t **tx_dst;
    int n_tx_dst;               /* staged frames that asked for tx_out */
    long long ticks;
    int rc;                     /* what the last tick's spangpu_echo_update_var() returned */
};

struct echo_can_state_s
{
    spangpu_echo_t *bank;
    int taps;
    int16_t *snapshot;          /* tap set 0 as echo_can_snapshot() last saw it */
    spangpu_echo_group_t *grp;  /* NULL: a private one-channel bank */
    int channel;
};

/* The tick's launch.  A tick that fails counts as a tick too. */
static int echo_group_run(grp_core_t *core)
{
    spangpu_echo_group_t *g = (spangpu_echo_group_t *) core;

    g->rc = spangpu_echo_update_var(g->bank, g->stage_tx, g->stage_rx, g->out_clean, (g->n_tx_dst)  ?  g->out_tx  :  NULL,
                                    SPANGPU_MEM_HOST, core->lens, g->hpf, core->max_samples, core->max_samples);
    g->n_tx_dst = 0;
    g->ticks++;
    return g->rc;
}

static void echo_group_deliver(grp_core_t *core)
{
    spangpu_echo_group_t *g = (spangpu_echo_group_t *) core;
    int c;

    for (c = 0;  c < core->n_ch;  c++)
    {
        if (core->run[c] == 0)
            continue;
        memcpy(g->clean_dst[c], g->out_clean + (size_t) c*core->max_samples, sizeof(int16_t)*core->run[c]);
        if (g->tx_dst[c])
            memcpy(g->tx_dst[c], g->out_tx + (size_t) c*core->max_samples, sizeof(int16_t)*core->run[c]);
    }
}

/* The object's channel is about to be read or changed: its staged frame, if it has one, runs first. */
static void echo_group_settle_locked(spangpu_echo_group_t *g, int channel)
{
    if (g->core.lens[channel])
        grp_flush_locked(&g->core);
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
    g->taps = taps;
    n = (size_t) n_channels*max_samples;
    g->stage_tx = (int16_t *) calloc(n, sizeof(int16_t));
    g->stage_rx = (int16_t *) calloc(n, sizeof(int16_t));
    g->out_clean = (int16_t *) calloc(n, sizeof(int16_t));
    g->out_tx = (int16_t *) calloc(n, sizeof(int16_t));
    g->hpf = (uint8_t *) calloc(n_channels, sizeof(uint8_t));
    g->clean_dst = (int16_t **) calloc(n_channels, sizeof(int16_t *));
    g->tx_dst = (int16_t **) calloc(n_channels, sizeof(int16_t *));
    if (grp_init(&g->core, n_channels, max_samples, echo_group_run, echo_group_deliver) < 0
        ||  g->stage_tx == NULL  ||  g->stage_rx == NULL  ||  g->out_clean == NULL  ||  g->out_tx == NULL
        ||  g->hpf == NULL  ||  g->clean_dst == NULL  ||  g->tx_dst == NULL)
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
    free(g->hpf);
    free(g->clean_dst);
    free(g->tx_dst);
    grp_free(&g->core);
    free(g);
    return SPANGPU_OK;
}

/* Returns what the tick's spangpu_echo_update_var() returned (0 when nothing was staged), not the number of frames as the
   other families' flush does. */
int spangpu_echo_group_flush(spangpu_echo_group_t *g)
{
    int rc;

    if (g == NULL)
        return SPANGPU_ERR_BAD_ARG;
    pthread_mutex_lock(&g->core.lock);
    g->rc = 0;
    grp_flush_locked(&g->core);
    rc = g->rc;
    pthread_mutex_unlock(&g->core.lock);
    return rc;
}

long long spangpu_echo_group_ticks(const spangpu_echo_group_t *g)
{
    spangpu_echo_group_t *m = (spangpu_echo_group_t *) g;       /* (the lock is not part of what const promises) */
    long long n;

    if (g == NULL)
        return 0;
    pthread_mutex_lock(&m->core.lock);
    n = m->ticks;
    pthread_mutex_unlock(&m->core.lock);
    return n;
}

spangpu_echo_t *spangpu_echo_group_bank(spangpu_echo_group_t *g)
{
    return (g)  ?  g->bank  :  NULL;
}

/* A claimed slot is a new canceller in the mode asked for; if the reset fails the attach is refused. */
static int echo_group_fresh(grp_core_t *core, int channel, void *adaption_mode)
{
    return (spangpu_echo_reset_channel(((spangpu_echo_group_t *) core)->bank, channel, *(int *) adaption_mode) == SPANGPU_OK)  ?  0  :  -1;
}

echo_can_state_t *spangpu_echo_can_attach(spangpu_echo_group_t *g, int channel, int adaption_mode)
{
    echo_can_state_t *ec;

    if (g == NULL  ||  channel < 0  ||  channel >= g->core.n_ch)
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
    if (grp_claim(&g->core, channel, ec, echo_group_fresh, &adaption_mode) < 0)
    {
        free(ec->snapshot);
        free(ec);
        return NULL;
    }
    return ec;
}

int spangpu_echo_can_pending(echo_can_state_t *ec)
{
    int rc;

    if (ec == NULL  ||  ec->grp == NULL)
        return 0;
    pthread_mutex_lock(&ec->grp->core.lock);
    rc = (ec->grp->core.lens[ec->channel] != 0);
    pthread_mutex_unlock(&ec->grp->core.lock);
    return rc;
}

/* The slot is released only if this object holds it (a tone group asks whether anybody does, the modem and line groups
   do not ask). */
static void echo_group_detach(echo_can_state_t *ec)
{
    spangpu_echo_group_t *g = ec->grp;
    int c = ec->channel;

    pthread_mutex_lock(&g->core.lock);
    if (g->core.handles[c] == ec)
    {
        if (g->core.lens[c]  &&  g->tx_dst[c])
            g->n_tx_dst--;
        grp_release(&g->core, c);
    }
    pthread_mutex_unlock(&g->core.lock);
}

/* Stage one object's frame (any thread); the tick runs when every attached object has staged, or in
   spangpu_echo_group_flush().  Returns SPANGPU_OK or an error code of include/spangpu.h (the other families' xxx_rx() say -1). */
static int echo_group_stage(echo_can_state_t *ec, const int16_t tx[], const int16_t rx[], int16_t clean[], int16_t tx_out[],
                            int n, int use_hpf_tx)
{
    spangpu_echo_group_t *g = ec->grp;
    int c = ec->channel;
    int rc;

    if (n > g->core.max_samples  ||  tx == NULL  ||  rx == NULL  ||  clean == NULL)
        return SPANGPU_ERR_BAD_ARG;
    if (grp_stage_begin(&g->core, c) < 0)
        return SPANGPU_ERR_STATE;       /* second frame before the tick ran */
    memcpy(g->stage_tx + (size_t) c*g->core.max_samples, tx, sizeof(int16_t)*n);
    memcpy(g->stage_rx + (size_t) c*g->core.max_samples, rx, sizeof(int16_t)*n);
    /* what goes with the frame is set under the lock that counts it: the tick reads every channel's flag */
    pthread_mutex_lock(&g->core.lock);
    g->hpf[c] = (use_hpf_tx)  ?  1  :  0;
    g->clean_dst[c] = clean;
    g->tx_dst[c] = tx_out;
    if (tx_out)
        g->n_tx_dst++;
    rc = grp_stage_commit(&g->core, c, n);
    pthread_mutex_unlock(&g->core.lock);
    return (rc > 0)  ?  SPANGPU_OK  :  rc;
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
        pthread_mutex_lock(&ec->grp->core.lock);
        echo_group_settle_locked(ec->grp, ec->channel);
    }
}

static void echo_leave(echo_can_state_t *ec)
{
    if (ec->grp)
        pthread_mutex_unlock(&ec->grp->core.lock);
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
        /* whatever the group has staged runs first, then this one sample as a tick of one channel: outside the staging
           protocol (nobody else's frame can be in `lens` while the lock is held), and not counted as a tick of the group */
        size_t at = (size_t) ec->channel*g->core.max_samples;

        pthread_mutex_lock(&g->core.lock);
        grp_flush_locked(&g->core);
        g->stage_tx[at] = tx;
        g->stage_rx[at] = rx;
        g->core.lens[ec->channel] = 1;
        g->hpf[ec->channel] = 0;
        if (spangpu_echo_update_var(g->bank, g->stage_tx, g->stage_rx, g->out_clean, NULL, SPANGPU_MEM_HOST, g->core.lens, g->hpf,
                                    g->core.max_samples, g->core.max_samples) == 1)
            clean = g->out_clean[at];
        g->core.lens[ec->channel] = 0;
        pthread_mutex_unlock(&g->core.lock);
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
        /* (as echo_can_update(): the group's staged frames first, then one sample of one channel under the group's lock) */
        pthread_mutex_lock(&ec->grp->core.lock);
        grp_flush_locked(&ec->grp->core);
        spangpu_echo_hpf_tx_channel(ec->bank, ec->channel, &tx, &out, 1);
        pthread_mutex_unlock(&ec->grp->core.lock);
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
