/*
 * shim_plc.c -- host side (plain C) of the spandsp-named entry points for packet loss concealment, declared in
 * include/spangpu_spandsp.h: plc_init, _release, _free, plc_rx and plc_fillin.  An object is a one-line concealment bank of
 * include/spangpu.h ("Packet loss concealment banks"), which works on the caller's samples in place.  Without a GPU plc_init()
 * returns NULL: there is no CPU implementation.
 */
#include "shim_object.h"

#define PIECE_SAMPLES   (1 << 20)       /* samples per launch of one object: a cut changes nothing but a gap's first overlap,
                                           which is 30 samples at the most */

plc_state_t *plc_init(plc_state_t *s)
{
    spangpu_plc_t *bank;

    if (spangpu_plc_create(&bank, 0, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, plc_state_t)) == NULL)
    {
        spangpu_plc_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    return s;
}

int plc_release(plc_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_plc_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int plc_free(plc_state_t *s)
{
    if (s)
    {
        plc_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

static int pieces(plc_state_t *s, int16_t amp[], int len, int32_t lost)
{
    int done = 0;

    if (s == NULL  ||  s->bank == NULL  ||  amp == NULL  ||  len <= 0)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE_SAMPLES)  ?  PIECE_SAMPLES  :  (len - done);

        if (spangpu_plc_run(s->bank, amp + done, SPANGPU_MEM_HOST, (long long) piece*2, NULL, &lost, piece) != SPANGPU_OK)
            break;
        done += piece;
    }
    return done;
}

int plc_rx(plc_state_t *s, int16_t amp[], int len)
{
    return pieces(s, amp, len, 0);
}

int plc_fillin(plc_state_t *s, int16_t amp[], int len)
{
    return pieces(s, amp, len, 1);
}
