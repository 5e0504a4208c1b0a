/* Two text telephones by their spandsp names, talking in both directions: A writes first, B answers once A has gone quiet.
   Every v18_tx() return value and every put_msg call goes to stdout, for tests/test_v18_c_gpu.py to hold against a
   recording of the reference doing the same. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define TICK        160
#define TICKS       420
#define ANSWER_AT   200

typedef struct
{
    char who;
    int tick;
} listener_t;

static void put_msg(void *user_data, const uint8_t *msg, int len)
{
    const listener_t *l = (const listener_t *) user_data;

    printf("m %c %d %d %d %d\n", l->who, l->tick, len, msg[0], msg[len]);
}

int main(int argc, char *argv[])
{
    const int mode = (argc > 1)  ?  (int) strtol(argv[1], NULL, 0)  :  V18_MODE_WEITBRECHT_5BIT_4545;
    listener_t la = {'A', 0};
    listener_t lb = {'B', 0};
    v18_state_t *a;
    v18_state_t *b;
    int16_t a_out[TICK];
    int16_t b_out[TICK];
    int t;

    if (v18_init(NULL, true, V18_MODE_DTMF, V18_AUTOMODING_NONE, put_msg, &la, NULL, NULL) != NULL
        ||  v18_init(NULL, true, mode, V18_AUTOMODING_USA, put_msg, &la, NULL, NULL) != NULL)
    {
        printf("v18_text: a mode or nation outside the text banks was taken\n");
        return 1;
    }
    a = v18_init(NULL, true, mode, V18_AUTOMODING_NONE, put_msg, &la, NULL, NULL);
    b = v18_init(NULL, false, mode | V18_MODE_REPETITIVE_SHIFTS_OPTION, V18_AUTOMODING_NONE, put_msg, &lb, NULL, NULL);
    if (a == NULL  ||  b == NULL)
    {
        printf("v18_text: v18_init failed: %s\n", spangpu_last_error());
        return 1;
    }
    printf("v18_text %s / %s, mode %d\n", v18_mode_to_str(v18_get_current_mode(a)), v18_status_to_str(V18_STATUS_SWITCH_TO_EDT),
           v18_get_current_mode(b));
    printf("p A %d\n", v18_put(a, "Hello B, 1 + 1?", -1));
    for (t = 0;  t < TICKS;  t++)
    {
        int na;
        int nb;

        la.tick = lb.tick = t;
        if (t == ANSWER_AT)
            printf("p B %d\n", v18_put(b, "Hi A: 2!xx", 8));
        memset(a_out, 0, sizeof(a_out));
        memset(b_out, 0, sizeof(b_out));
        na = v18_tx(a, a_out, TICK);
        nb = v18_tx(b, b_out, TICK);
        if (na  ||  nb)
            printf("t %d %d %d\n", t, na, nb);
        v18_rx(a, b_out, TICK);
        v18_rx(b, a_out, TICK);
    }
    v18_free(a);
    v18_free(b);
    return 0;
}
