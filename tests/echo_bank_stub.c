/* A stand-in for the echo canceller bank behind csrc/shim_echo.c, for the host-side thread-safety test of the echo groups
 * (tests/test_echo_group_c_gpu.py: shim_echo.c + this file + tests/c_callers/echo_group.c under -fsanitize=thread; no GPU).
 * It keeps no canceller: clean = rx/2 + tx/64, for the rows of the channels that take part -- and it touches exactly the
 * memory the real bank touches, which is what the sanitizer watches.  Test code only. */
#include <stdlib.h>
#include <string.h>

#include "spangpu.h"

struct spangpu_echo_s
{
    int n_ch;
    int taps;
    int *mode;
};

const char *spangpu_last_error(void) { return "stub bank"; }

int spangpu_echo_create(spangpu_echo_t **ec, int device, int n_channels, int taps, int adaption_mode)
{
    spangpu_echo_t *e;
    int c;

    (void) device;
    if ((e = (spangpu_echo_t *) calloc(1, sizeof(*e))) == NULL  ||  (e->mode = (int *) calloc((size_t) n_channels, sizeof(int))) == NULL)
        return SPANGPU_ERR_NO_MEMORY;
    e->n_ch = n_channels;
    e->taps = taps;
    for (c = 0;  c < n_channels;  c++)
        e->mode[c] = adaption_mode;
    *ec = e;
    return SPANGPU_OK;
}

int spangpu_echo_destroy(spangpu_echo_t *e)
{
    if (e)
    {
        free(e->mode);
        free(e);
    }
    return SPANGPU_OK;
}

int spangpu_echo_update_var(spangpu_echo_t *e, const int16_t *tx, const int16_t *rx, int16_t *clean, int16_t *tx_out,
                            int mem, const int32_t *lens, const uint8_t *use_hpf_tx, int max_samples, long long stride)
{
    int c;
    int i;
    int n = 0;

    (void) mem;
    (void) use_hpf_tx;
    (void) max_samples;
    for (c = 0;  c < e->n_ch;  c++)
    {
        if (lens[c] <= 0)
            continue;
        n++;
        for (i = 0;  i < lens[c];  i++)
        {
            clean[c*stride + i] = (int16_t) (rx[c*stride + i]/2 + tx[c*stride + i]/64);
            if (tx_out)
                tx_out[c*stride + i] = tx[c*stride + i];
        }
    }
    return n;
}

int spangpu_echo_update_tx(spangpu_echo_t *e, const int16_t *tx, const int16_t *rx, int16_t *clean, int16_t *tx_out,
                           int mem, int samples, long long stride, int use_hpf_tx)
{
    int c;
    int i;

    (void) mem;
    (void) use_hpf_tx;
    for (c = 0;  c < e->n_ch;  c++)
    {
        for (i = 0;  i < samples;  i++)
        {
            clean[c*stride + i] = (int16_t) (rx[c*stride + i]/2 + tx[c*stride + i]/64);
            if (tx_out)
                tx_out[c*stride + i] = tx[c*stride + i];
        }
    }
    return 0;
}

int spangpu_echo_update(spangpu_echo_t *e, const int16_t *tx, const int16_t *rx, int16_t *clean,
                        int mem, int samples, long long stride, int use_hpf_tx)
{
    return spangpu_echo_update_tx(e, tx, rx, clean, NULL, mem, samples, stride, use_hpf_tx);
}

int spangpu_echo_hpf_tx(spangpu_echo_t *e, const int16_t *tx, int16_t *out, int samples, long long stride)
{
    int c;

    for (c = 0;  c < e->n_ch;  c++)
        memmove(out + c*stride, tx + c*stride, sizeof(int16_t)*(size_t) samples);
    return 0;
}

int spangpu_echo_hpf_tx_channel(spangpu_echo_t *e, int channel, const int16_t *tx, int16_t *out, int samples)
{
    (void) e;
    (void) channel;
    memmove(out, tx, sizeof(int16_t)*(size_t) samples);
    return 0;
}

int spangpu_echo_adaption_mode(spangpu_echo_t *e, int channel, int adaption_mode)
{
    e->mode[channel] = adaption_mode;
    return SPANGPU_OK;
}

int spangpu_echo_reset_channel(spangpu_echo_t *e, int channel, int adaption_mode)
{
    e->mode[channel] = adaption_mode;
    return SPANGPU_OK;
}

int spangpu_echo_flush(spangpu_echo_t *e, int channel)
{
    (void) e;
    (void) channel;
    return SPANGPU_OK;
}

int spangpu_echo_get_state(spangpu_echo_t *e, int channel, int32_t *scalars, int32_t *taps32, int16_t *taps16, int16_t *history)
{
    (void) channel;
    (void) scalars;
    (void) taps32;
    (void) history;
    if (taps16)
        memset(taps16, 0, sizeof(int16_t)*4*(size_t) e->taps);
    return SPANGPU_OK;
}
