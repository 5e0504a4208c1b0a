/*
 * adsi_host.c -- the host-only parts of the caller-ID (ADSI) banks, plain C with no HIP in it: message packing, the field
 * helpers, the ITU CRC-16 and the standards' names (include/spangpu.h, "Caller-ID banks").  The C ABI unit (adsi_api.hip) and
 * the spandsp-named entry points (shim_adsi.c) both use it, and a stand-alone program can link it alone.
 *
 * What is restated (paths relative to the reference tree):
 *   adsi_tx_put_message(), the packing part    src/adsi.c:647-717
 *   adsi_next_field()                          src/adsi.c:961-1097
 *   adsi_add_field()                           src/adsi.c:1100-1214      adsi_encode_baudot() :773-933 as a table built here
 *   adsi_standard_to_str()                     src/adsi.c:1217-1237
 *   crc_itu16_calc()                           src/crc.c:161-169, bit by bit (polynomial 0x8408, reflected)
 */
#include <stddef.h>
#include <string.h>

#include "spangpu.h"

#define DLE     0x10
#define SOH     0x01
#define STX     0x02
#define ETX     0x03

uint16_t spangpu_adsi_crc16(const uint8_t *buf, int len, uint16_t crc)
{
    int i;
    int k;

    for (i = 0;  i < len;  i++)
    {
        crc ^= buf[i];
        for (k = 0;  k < 8;  k++)
            crc = (crc & 1)  ?  (uint16_t) ((crc >> 1) ^ 0x8408)  :  (uint16_t) (crc >> 1);
    }
    return crc;
}

int spangpu_adsi_pack_message(int standard, const uint8_t *msg, int len, uint8_t *out, int out_len)
{
    int i;
    int j;
    int sum;
    uint16_t crc;

    if (standard < SPANGPU_ADSI_STANDARD_CLASS  ||  standard > SPANGPU_ADSI_STANDARD_JCLIP  ||  msg == NULL  ||  out == NULL
        ||  len < 2  ||  out_len < SPANGPU_ADSI_MSG_BYTES)
        return SPANGPU_ERR_BAD_ARG;
    if (standard == SPANGPU_ADSI_STANDARD_JCLIP)
    {
        if (len > 128 - 9)
            return -1;
        i = 0;
        out[i++] = DLE;
        out[i++] = SOH;
        out[i++] = 0x07;
        out[i++] = DLE;
        out[i++] = STX;
        out[i++] = msg[0];
        out[i++] = (uint8_t) (len - 2);
        /* only the overall length is stuffed here; the fields were stuffed as they were added */
        if (len - 2 == DLE)
            out[i++] = DLE;
        memcpy(&out[i], &msg[2], (size_t) (len - 2));
        i += len - 2;
        out[i++] = DLE;
        out[i++] = ETX;
        /* bit 7 becomes the sum, modulo 2, of bits 0 to 6 */
        for (j = 0;  j < i;  j++)
        {
            int b = out[j] & 0x7F;
            int p = b;

            p ^= p >> 4;
            p ^= p >> 2;
            p ^= p >> 1;
            out[j] = (uint8_t) (b | ((p & 1) << 7));
        }
        crc = spangpu_adsi_crc16(out + 2, i - 2, 0);
        out[i++] = (uint8_t) (crc & 0xFF);
        out[i++] = (uint8_t) ((crc >> 8) & 0xFF);
        return i;
    }
    if (len > 255)
        return -1;
    memcpy(out, msg, (size_t) len);
    out[1] = (uint8_t) (len - 2);
    sum = 0;
    for (i = 0;  i < len;  i++)
        sum += out[i];
    out[len] = (uint8_t) ((-sum) & 0xFF);
    return len + 1;
}

int spangpu_adsi_next_field(int standard, const uint8_t *msg, int msg_len, int pos, uint8_t *field_type, const uint8_t **field_body,
                            int *field_len)
{
    int i;

    switch (standard)
    {
    case SPANGPU_ADSI_STANDARD_CLASS:
    case SPANGPU_ADSI_STANDARD_CLIP:
    case SPANGPU_ADSI_STANDARD_ACLIP:
        if (pos >= msg_len)
            return -1;
        if (pos <= 0)
        {
            /* the message type */
            *field_type = msg[0];
            *field_len = 0;
            *field_body = NULL;
            pos = 2;
        }
        else
        {
            if ((msg[0] & 0x80))
            {
                /* multiple data message format: type, length, contents.  (A lone type byte at the end: the reference reads
                   the byte behind the message as its length and then answers -2 whatever it read.) */
                if (pos + 2 > msg_len)
                    return -2;
                *field_type = msg[pos++];
                *field_len = msg[pos++];
                *field_body = msg + pos;
            }
            else
            {
                /* single data message format: the rest is one field */
                *field_type = 0;
                *field_len = msg_len - pos;
                *field_body = msg + pos;
            }
            pos += *field_len;
        }
        if (pos > msg_len)
            return -2;
        break;
    case SPANGPU_ADSI_STANDARD_JCLIP:
        if (pos >= msg_len - 2)
            return -1;
        /* (every read below stays inside the message: a position that has run past it answers -2 in the reference, too,
           after it has read what lies behind) */
        if (pos <= 0)
        {
            pos = 5;
            if (msg_len < 9)
                return -2;
            *field_type = msg[pos++];
            if (*field_type == DLE)
                pos++;
            if (msg[pos++] == DLE)
                pos++;
            *field_len = 0;
            *field_body = NULL;
        }
        else
        {
            *field_type = msg[pos++];
            if (*field_type == DLE)
                pos++;
            if (pos >= msg_len)
                return -2;
            *field_len = msg[pos++];
            if (*field_len == DLE)
                pos++;
            *field_body = msg + pos;
            pos += *field_len;
        }
        if (pos > msg_len - 2)
            return -2;
        break;
    case SPANGPU_ADSI_STANDARD_CLIP_DTMF:
        if (pos > msg_len)
            return -1;
        if (pos <= 0)
        {
            pos = 1;
            *field_type = msg[msg_len - 1];
            *field_len = 0;
            *field_body = NULL;
        }
        else
        {
            /* positions are handed out one up, so that the first field's is not 0 */
            pos--;
            if (msg[pos] >= '0'  &&  msg[pos] <= '9')
                *field_type = 0;
            else
                *field_type = msg[pos++];
            *field_body = msg + pos;
            i = pos;
            while (i < msg_len  &&  msg[i] >= '0'  &&  msg[i] <= '9')
                i++;
            *field_len = i - pos;
            pos = i;
            if (pos < msg_len  &&  (msg[pos] == '#'  ||  msg[pos] == 'C'))
                pos++;
            if (pos > msg_len)
                return -2;
            pos++;
        }
        break;
    case SPANGPU_ADSI_STANDARD_TDD:
        if (pos >= msg_len)
            return -1;
        *field_type = 0;
        *field_body = msg;
        *field_len = msg_len;
        pos = msg_len;
        break;
    }
    return pos;
}

/* The 5-bit code of a character and its set: 0xFF none, 0x40 | code in both sets, 0x80 | code figures, code letters. */
static int baudot_of(int ch)
{
    static const char letters[33] = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\0MXV";
    static const char figures[33] = "\0003\n- '87\r$4*,\0:(5+)2#6019?\0^./=";
    int c;

    ch &= 0x7F;
    if (ch == 0)
        return 0x00;
    if (ch == '\n')
        return 0x42;
    if (ch == '\r')
        return 0x48;
    if (ch == ' ')
        return 0x44;
    if (ch >= 'a'  &&  ch <= 'z')
        ch -= 'a' - 'A';
    for (c = 1;  c < 32;  c++)
    {
        if (letters[c] == ch)
            return c;
        if (figures[c] == ch)
            return 0x80 | c;
    }
    return 0xFF;
}

int spangpu_adsi_add_field(int standard, int *baudot_shift, uint8_t *msg, int len, uint8_t field_type, const uint8_t *field_body,
                           int field_len)
{
    int i;
    int x;

    switch (standard)
    {
    case SPANGPU_ADSI_STANDARD_CLASS:
    case SPANGPU_ADSI_STANDARD_CLIP:
    case SPANGPU_ADSI_STANDARD_ACLIP:
        if (len <= 0)
        {
            /* a new message: the field type is the message type */
            msg[0] = field_type;
            msg[1] = 0;
            len = 2;
        }
        else
        {
            if (field_type)
            {
                msg[len++] = field_type;
                msg[len++] = (uint8_t) field_len;
                if (field_len == DLE)
                    msg[len++] = (uint8_t) field_len;
            }
            memcpy(&msg[len], field_body, (size_t) field_len);
            len += field_len;
        }
        break;
    case SPANGPU_ADSI_STANDARD_JCLIP:
        if (len <= 0)
        {
            msg[0] = field_type;
            msg[1] = 0;
            len = 2;
        }
        else
        {
            /* every DLE goes out twice */
            msg[len++] = field_type;
            if (field_type == DLE)
                msg[len++] = field_type;
            msg[len++] = (uint8_t) field_len;
            if (field_len == DLE)
                msg[len++] = (uint8_t) field_len;
            for (i = 0;  i < field_len;  i++)
            {
                msg[len++] = field_body[i];
                if (field_body[i] == DLE)
                    msg[len++] = field_body[i];
            }
        }
        break;
    case SPANGPU_ADSI_STANDARD_CLIP_DTMF:
        if (len <= 0)
        {
            msg[0] = field_type;
            len = 1;
        }
        else
        {
            /* the terminator, which is the message type, moves to the new end */
            x = msg[--len];
            if (field_type != 0)
                msg[len++] = field_type;
            memcpy(&msg[len], field_body, (size_t) field_len);
            msg[len + field_len] = (uint8_t) x;
            len += field_len + 1;
        }
        break;
    case SPANGPU_ADSI_STANDARD_TDD:
        if (len < 0)
            len = 0;
        for (i = 0;  i < field_len;  i++)
        {
            const int e = baudot_of(field_body[i]);
            int shifted = 0;

            if (e == 0xFF)
                continue;
            x = e & 0x1F;
            if (!(e & 0x40)  &&  baudot_shift)
            {
                const int set = (e & 0x80)  ?  1  :  0;

                if (*baudot_shift != set)
                {
                    *baudot_shift = set;
                    msg[len++] = (uint8_t) (set  ?  0x1B  :  0x1F);
                    shifted = 1;
                }
            }
            /* (code 0 with no shift ahead of it is "nothing to send" in the reference, too) */
            if (x  ||  shifted)
                msg[len++] = (uint8_t) x;
        }
        break;
    }
    return len;
}

const char *spangpu_adsi_standard_to_str(int standard)
{
    static const char *const names[] = {"CLASS", "CLIP", "A-CLIP", "J-CLIP", "CLIP-DTMF", "TDD"};

    if (standard < SPANGPU_ADSI_STANDARD_CLASS  ||  standard > SPANGPU_ADSI_STANDARD_TDD)
        return "???";
    return names[standard - 1];
}
