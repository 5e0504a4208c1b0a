/* A caller-ID sender and receiver by their spandsp names (include/spangpu_spandsp.h), per standard: adsi_tx_init ->
 * adsi_add_field -> adsi_tx_put_message -> adsi_tx / adsi_rx in 160-sample calls with a counting put_msg, then the fields of
 * what arrived through adsi_next_field.  Prints one line per delivered message; the two standards outside the banks must
 * give NULL from both inits. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define TICK 160

static int delivered;
static uint8_t last[256];
static int last_len;

static void put_msg(void *user_data, const uint8_t *msg, int len)
{
    (void) user_data;
    delivered++;
    last_len = len;
    memcpy(last, msg, (size_t) len);
}

static int one(int standard)
{
    adsi_tx_state_t tx_store;
    adsi_tx_state_t *tx = adsi_tx_init(&tx_store, standard);
    adsi_rx_state_t *rx = adsi_rx_init(NULL, standard, put_msg, NULL);
    uint8_t msg[64];
    int16_t amp[TICK];
    uint8_t type;
    const uint8_t *body;
    int flen;
    int len;
    int pos;
    int t;

    if (tx == NULL  ||  rx == NULL)
    {
        fprintf(stderr, "init failed for %s\n", adsi_standard_to_str(standard));
        return 1;
    }
    len = adsi_add_field(tx, msg, -1, (standard == ADSI_STANDARD_JCLIP)  ?  JCLIP_MDMF_CALLERID  :  CLASS_MDMF_CALLERID, NULL, 0);
    len = adsi_add_field(tx, msg, len, MCLASS_CALLER_NUMBER, (const uint8_t *) "5551212", 7);
    delivered = 0;
    adsi_tx_send_alert_tone(tx);
    if (adsi_tx_put_message(tx, msg, len) != len  ||  adsi_tx_put_message(tx, msg, len) != 0)
        return 1;
    for (t = 0;  t < 80;  t++)
    {
        const int got = adsi_tx(tx, amp, TICK);

        memset(amp + got, 0, (size_t) (TICK - got)*sizeof(int16_t));
        adsi_rx(rx, amp, TICK);
    }
    printf("%s %d", adsi_standard_to_str(standard), delivered);
    pos = -1;
    while (delivered == 1  &&  (pos = adsi_next_field(rx, last, last_len, pos, &type, &body, &flen)) > 0)
    {
        printf(" %02x:%d", type, flen);
        if (body)
            printf(":%.*s", flen, (const char *) body);
    }
    printf("\n");
    adsi_tx_release(tx);
    adsi_tx_free(tx);
    adsi_rx_free(rx);
    return delivered != 1;
}

int main(void)
{
    int bad = 0;
    int s;

    for (s = ADSI_STANDARD_CLASS;  s <= ADSI_STANDARD_JCLIP;  s++)
        bad |= one(s);
    for (s = ADSI_STANDARD_CLIP_DTMF;  s <= ADSI_STANDARD_TDD;  s++)
        printf("%s %s %s\n", adsi_standard_to_str(s), adsi_tx_init(NULL, s)  ?  "object"  :  "NULL", adsi_rx_init(NULL, s, put_msg, NULL)  ?  "object"  :  "NULL");
    return bad;
}
