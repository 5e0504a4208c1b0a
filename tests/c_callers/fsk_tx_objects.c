/* fsk_tx, modem_connect_tones_tx and async_tx objects by name, as a strict C99 caller sees them: a counting get_bit and a
 * status handler on a V.23 channel 1 sender with three data bits and then SIG_STATUS_END_OF_DATA -- the call returns 26
 * samples after 4 get_bit calls, the handler hears END_OF_DATA then SHUTDOWN_COMPLETE, the next call returns 0 and asks
 * for nothing -- then a restart, a framed V.21 sender fed by async_tx_get_bit, and a finite answer tone. */
#include <stdio.h>
#include <string.h>

#include "spangpu_spandsp.h"

static int calls;
static int bits_left;
static int statuses[8];
static int n_status;

static int get_bit(void *user_data)
{
    (void) user_data;
    calls++;
    if (bits_left <= 0)
        return SIG_STATUS_END_OF_DATA;
    bits_left--;
    return bits_left & 1;
}

static void status(void *user_data, int s)
{
    (void) user_data;
    if (n_status < 8)
        statuses[n_status++] = s;
}

static const uint8_t text[] = "Hi";
static int text_at;

static int get_byte(void *user_data)
{
    (void) user_data;
    return (text_at < 2)  ?  (int) text[text_at++]  :  (int) SIG_STATUS_LINK_IDLE;
}

#define CHECK(x) do { if (!(x)) { printf("fsk_tx_objects: FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(void)
{
    int16_t amp[400];
    fsk_tx_state_t *tx;
    fsk_tx_state_t mine;
    async_tx_state_t *as;
    modem_connect_tones_tx_state_t *ans;
    int i;
    int n;
    int total;

    /* V.23 ch 1: a bit boundary at samples 6, 13, 19, 26: three bits, then the end of the data */
    bits_left = 3;
    tx = fsk_tx_init(NULL, &preset_fsk_specs[2], get_bit, NULL);
    CHECK(tx != NULL);
    fsk_tx_set_modem_status_handler(tx, status, NULL);
    for (i = 0;  i < 400;  i++)
        amp[i] = 12345;
    n = fsk_tx(tx, amp, 160);
    CHECK(n == 26  &&  calls == 4);
    CHECK(n_status == 2  &&  statuses[0] == SIG_STATUS_END_OF_DATA  &&  statuses[1] == SIG_STATUS_SHUTDOWN_COMPLETE);
    CHECK(amp[0] == 0  &&  amp[1] != 0  &&  amp[25] != 12345  &&  amp[26] == 12345  &&  amp[159] == 12345);
    CHECK(fsk_tx(tx, amp, 160) == 0  &&  calls == 4  &&  n_status == 2);
    /* a restart revives it: 20 samples of V.23 ch 1 ask for exactly 3 bits */
    CHECK(fsk_tx_restart(tx, &preset_fsk_specs[2]) == 0);
    bits_left = 100;
    calls = 0;
    CHECK(fsk_tx(tx, amp, 19) == 19  &&  calls == 2);
    CHECK(fsk_tx(tx, amp, 1) == 1  &&  calls == 3);
    fsk_tx_power(tx, -20.0f);
    fsk_tx_set_get_bit(tx, get_bit, NULL);
    CHECK(fsk_tx(tx, amp, 400) == 400  &&  calls == 63);
    CHECK(fsk_tx_free(tx) == 0);

    /* caller storage, bits from the async framer: 2 characters of 10 bits at 300 baud, then idle marks */
    as = async_tx_init(NULL, 8, ASYNC_PARITY_NONE, 1, false, get_byte, NULL);
    CHECK(as != NULL);
    async_tx_presend_bits(as, 2);
    CHECK(fsk_tx_init(&mine, &preset_fsk_specs[1], async_tx_get_bit, as) == &mine);
    total = 0;
    for (i = 0;  i < 5;  i++)
        total += fsk_tx(&mine, amp, 160);
    CHECK(total == 800  &&  text_at == 2);
    CHECK(fsk_tx_release(&mine) == 0  &&  async_tx_release(as) == 0  &&  async_tx_free(as) == 0);

    /* ANS: 22400 samples in all, whatever is asked for */
    CHECK(modem_connect_tones_tx_init(NULL, MODEM_CONNECT_TONES_FAX_PREAMBLE) == NULL);
    ans = modem_connect_tones_tx_init(NULL, MODEM_CONNECT_TONES_ANS);
    CHECK(ans != NULL);
    total = 0;
    for (i = 0;  i < 60;  i++)
    {
        n = modem_connect_tones_tx(ans, amp, 400);
        CHECK(n == ((i < 56)  ?  400  :  0));
        total += n;
    }
    CHECK(total == 22400);
    CHECK(modem_connect_tones_tx_release(ans) == 0  &&  modem_connect_tones_tx_free(ans) == 0);
    printf("fsk_tx_objects: ok\n");
    return 0;
}
