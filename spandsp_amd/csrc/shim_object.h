/*
 * shim_object.h -- what every lone object behind include/spangpu_spandsp.h does, written once: an object that owns a private
 * one-channel bank (the codecs, v18, adsi_*, the FSK, connect tone, modem and digit senders).  Static functions, included by
 * each shim: nothing here is exported, and nothing here touches a bank -- the two loops are macros that make a function around
 * the family's own bank calls, so that those stay typed calls at the place that names them.
 *
 * A state struct embeds a spangpu_object_t (spangpu_spandsp.h) as `obj`.  What a family does differently is a parameter or
 * stays at its call site: which bank it makes and destroys, the length it trims in front, its piece, its element size, what it
 * does when the data ends.
 *
 * Behaviours this sharing makes uniform:
 *  - a failed xxx_init() leaves caller-supplied storage exactly as it was, as the reference's do: the family makes its bank
 *    first and calls obj_take() only once it exists.  (fsk_tx, modem_connect_tones_tx, dtmf_tx, bell_mf_tx, r2_mf_tx and the
 *    modem senders used to zero the storage and then fail.)
 *  - the row's capacity is in bytes and a size_t everywhere.
 */
#ifndef SHIM_OBJECT_H
#define SHIM_OBJECT_H

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

/* The object's storage, zeroed: the caller's, or `size` bytes of the heap (NULL: none to be had; the family destroys its
   bank).  `at` is where the spangpu_object_t lies in it. */
static inline void *obj_take(void *storage, size_t size, size_t at)
{
    const int mine = (storage != NULL);

    if (mine)
        memset(storage, 0, size);
    else if ((storage = calloc(1, size)) == NULL)
        return NULL;
    ((spangpu_object_t *) ((char *) storage + at))->caller_storage = mine;
    return storage;
}
#define OBJ_TAKE(s, T)      ((T *) obj_take(s, sizeof(T), offsetof(T, obj)))

/* xxx_release(): obj_drop(&s->obj, NULL) once the bank is gone.  xxx_free(): obj_drop(&s->obj, s) after xxx_release(). */
static inline void obj_drop(spangpu_object_t *o, void *storage)
{
    free(o->row);
    o->row = NULL;
    o->row_cap = 0;
    if (storage  &&  !o->caller_storage)
        free(storage);
}

/* The row, grown to `bytes` if it is smaller; NULL: no memory */
static inline void *obj_room(spangpu_object_t *o, size_t bytes)
{
    if (o->row_cap < bytes)
    {
        void *r = realloc(o->row, bytes);

        if (r == NULL)
            return NULL;
        o->row = r;
        o->row_cap = bytes;
    }
    return o->row;
}

/* A codec call, cut into launches of at most `most` items: name(o, bank, in, in_el, out, out_el, len, most) takes `len` items
   of in_el bytes and returns how many of out_el bytes `out` got.  The bank writes a row of its capacity; the caller's buffer
   holds what the reference would write. */
#define OBJ_CODEC_LOOP(name, bank_t, capacity, code)                                                                    \
static int name(spangpu_object_t *o, bank_t *bank, const void *in, size_t in_el, void *out, size_t out_el, int len, int most)    \
{                                                                                                                       \
    int done = 0;                                                                                                       \
    int total = 0;                                                                                                      \
                                                                                                                        \
    while (done < len)                                                                                                  \
    {                                                                                                                   \
        const int piece = (len - done > most)  ?  most  :  (len - done);                                                \
        const long long cap = capacity(bank, piece);                                                                    \
        int32_t got = 0;                                                                                                \
                                                                                                                        \
        if (cap <= 0  ||  obj_room(o, (size_t) cap*out_el) == NULL)                                                     \
            break;                                                                                                      \
        if (code(bank, (const uint8_t *) in + (size_t) done*in_el, SPANGPU_MEM_HOST, (long long) ((size_t) piece*in_el), NULL, piece,   \
                 o->row, SPANGPU_MEM_HOST, (long long) ((size_t) cap*out_el), &got) != SPANGPU_OK)                      \
            break;                                                                                                      \
        memcpy((uint8_t *) out + (size_t) total*out_el, o->row, (size_t) got*out_el);                                   \
        total += got;                                                                                                   \
        done += piece;                                                                                                  \
    }                                                                                                                   \
    return total;                                                                                                       \
}

/* A sender call, cut into launches of at most `most` samples, over when a launch makes less than it was asked for.  The bank
   fills a row with zeros behind what it made; the reference leaves the caller's samples there alone. */
#define OBJ_SENDER_LOOP(name, bank_t, tx)                                                                               \
static int name(spangpu_object_t *o, bank_t *bank, int16_t amp[], int max_len, int most)                                \
{                                                                                                                       \
    int done = 0;                                                                                                       \
                                                                                                                        \
    while (done < max_len)                                                                                              \
    {                                                                                                                   \
        const int piece = (max_len - done > most)  ?  most  :  (max_len - done);                                        \
        int32_t got = 0;                                                                                                \
                                                                                                                        \
        if (obj_room(o, (size_t) piece*sizeof(int16_t)) == NULL                                                         \
            ||  tx(bank, SPANGPU_MEM_HOST, (int16_t *) o->row, piece, piece, &got) != SPANGPU_OK)                       \
            break;                                                                                                      \
        memcpy(amp + done, o->row, (size_t) got*sizeof(int16_t));                                                       \
        done += got;                                                                                                    \
        if (got < piece)                                                                                                \
            break;                                                                                                      \
    }                                                                                                                   \
    return done;                                                                                                        \
}

/* Ask the caller's get_bit for the `due` bits a launch needs, in order, and pack them LSB first into bits[bytes]; returns how
   many came before SIG_STATUS_END_OF_DATA, which sets *ended and ends the asking. */
static inline int32_t obj_pull_bits(span_get_bit_func_t get_bit, void *user_data, long long due, uint8_t *bits, size_t bytes, int *ended)
{
    int32_t n_bits = 0;

    memset(bits, 0, bytes);
    *ended = 0;
    while (n_bits < due)
    {
        const int bit = get_bit(user_data);

        if (bit == SIG_STATUS_END_OF_DATA)
        {
            *ended = 1;
            break;
        }
        bits[n_bits >> 3] |= (uint8_t) ((bit & 1) << (n_bits & 7));
        n_bits++;
    }
    return n_bits;
}

#endif
