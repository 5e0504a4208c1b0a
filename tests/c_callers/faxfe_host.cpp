// faxfe_host.cpp -- the per-channel functions of spandsp_amd/csrc/faxfe_dev.hpp compiled for the host and run one lane at a
// time over every case of tests/golden/faxfe.npz (tests/test_faxfe.py writes the cases out as whitespace separated
// integers and builds this file with -fsanitize=address,undefined).  The receivers do not run here: each tick's two event
// rows are the fixture's, as the reference's own receivers delivered them under the handler of that tick.  Exit status 0 and
// "ok ..." on the last line: every tick's records, octets, non-ECM bits, handler and rx_frame_received equal the
// reference's, and so do the dc_restore state and the framer's words and buffer at the end.
//
//   faxfe_host <cases file>
//
// The file: records that start with a letter.
//   C use_dc ticks n_ops
//     n_ops x: tick call which bit_rate short_train hdlc_mode          call 1: start_slow_modem, 2: start_fast_modem
//     ticks x: len samples.., n_fast events.., n_v21 events.., handler rx_frame_received, n_recs records.., n_bytes octets..,
//              n_put values..
//     dc_state, 18 framer words, 404 buffer octets
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define SPG_HDLC_STEP_FUNCTIONS_ONLY
#include "../../spandsp_amd/csrc/faxfe_dev.hpp"

using namespace spg;

static FILE *in;

static int next_int()
{
    int v;
    if (fscanf(in, "%d", &v) != 1)
    {
        fprintf(stderr, "cases file cut short\n");
        exit(2);
    }
    return v;
}

static void fail(const char *what, int case_no, int tick, long long got, long long want)
{
    fprintf(stderr, "case %d tick %d: %s: got %lld, reference %lld\n", case_no, tick, what, got, want);
    exit(1);
}

// the words' side of the two control calls, as faxfe_api.hip keeps it (the receivers' side is not this program's)
static void control(int32_t *fe, int call, int which, int bit_rate, int short_train, int hdlc_mode)
{
    if (call == 1)
    {
        fe[FE_HANDLER] = kFaxFeV21Only;
        fe[FE_RX_FRAME_RECEIVED] = 0;
        return;
    }
    fe[FE_SHORT_TRAIN] = (fe[FE_FAST_MODEM] != which)  ?  0  :  (short_train  ?  1  :  0);
    fe[FE_HANDLER] = kFaxFeFastAndV21;
    fe[FE_FAST_MODEM] = which;
    fe[FE_BIT_RATE] = bit_rate;
    fe[FE_HDLC_MODE] = hdlc_mode  ?  1  :  0;
    fe[FE_RX_FRAME_RECEIVED] = 0;
}

static long long one_case(int case_no)
{
    const int use_dc = next_int();
    const int ticks = next_int();
    const int n_ops = next_int();
    std::vector<int> ops((size_t) n_ops*6);
    for (int &v : ops)
        v = next_int();
    int32_t fe[kFaxFeWords];
    memset(fe, 0, sizeof(fe));
    fe[FE_SLOT] = -1;
    int32_t w[kHdlcRxWords];
    hdlc_rx_words_init(w, 0, 1, 5);
    // exactly the buffer's and the rows' sizes: a step outside them is the sanitizer's to find
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    long long checked = 0;
    for (int t = 0;  t < ticks;  t++)
    {
        for (int k = 0;  k < n_ops;  k++)
        {
            if (ops[6*k] == t)
                control(fe, ops[6*k + 1], ops[6*k + 2], ops[6*k + 3], ops[6*k + 4], ops[6*k + 5]);
        }
        const int len = next_int();
        std::vector<int16_t> amp(len);
        for (int16_t &v : amp)
            v = (int16_t) next_int();
        if (use_dc  &&  fe[FE_HANDLER] != kFaxFeNone)
        {
            for (int16_t &v : amp)
                v = faxfe_dc_restore(&fe[FE_DC_STATE], v);
        }
        std::vector<int8_t> fast(next_int());
        for (int8_t &v : fast)
            v = (int8_t) next_int();
        std::vector<int16_t> v21(next_int());
        for (int16_t &v : v21)
            v = (int16_t) next_int();
        long long rec_cap;
        long long byte_cap;
        hdlc_rx_capacity((long long) (fast.size() + v21.size()), &rec_cap, &byte_cap);
        std::vector<int32_t> recs(rec_cap);
        std::vector<uint8_t> bytes(byte_cap);
        std::vector<int8_t> put(fast.size());
        HdlcRxSink out;
        out.recs = recs.data();
        out.bytes = bytes.data();
        out.rec_cap = (int) rec_cap;
        out.byte_cap = (int) byte_cap;
        out.n_recs = 0;
        out.n_bytes = 0;
        FaxFeRows r;
        r.fast = fast.data();
        r.n_fast = (int) fast.size();
        r.v21 = v21.data();
        r.n_v21 = (int) v21.size();
        r.put = put.data();
        r.put_cap = (int) put.size();
        r.n_put = 0;
        HdlcBuf buf;
        buf.open(frame.data(), 1);
        if (fe[FE_HANDLER] != kFaxFeNone)
            faxfe_route_channel(fe, w, buf, out, r);
        buf.close();

        const int handler = next_int();
        if (fe[FE_HANDLER] != handler)
            fail("handler", case_no, t, fe[FE_HANDLER], handler);
        const int frx = next_int();
        if (fe[FE_RX_FRAME_RECEIVED] != frx)
            fail("rx_frame_received", case_no, t, fe[FE_RX_FRAME_RECEIVED], frx);
        int n = next_int();
        if (out.n_recs != n  ||  n > rec_cap)
            fail("records", case_no, t, out.n_recs, n);
        for (int i = 0;  i < n;  i++)
        {
            const int want = next_int();
            if (recs[i] != want)
                fail("a record", case_no, t, recs[i], want);
        }
        checked += n;
        n = next_int();
        if (out.n_bytes != n  ||  n > byte_cap)
            fail("octets", case_no, t, out.n_bytes, n);
        for (int i = 0;  i < n;  i++)
        {
            const int want = next_int();
            if (bytes[i] != want)
                fail("an octet", case_no, t, bytes[i], want);
        }
        checked += n;
        n = next_int();
        if (r.n_put != n  ||  n > r.put_cap)
            fail("non-ECM put_bit calls", case_no, t, r.n_put, n);
        for (int i = 0;  i < n;  i++)
        {
            const int want = next_int();
            if (put[i] != want)
                fail("a non-ECM put_bit", case_no, t, put[i], want);
        }
        checked += n + 2;
    }
    const int dc = next_int();
    if (fe[FE_DC_STATE] != dc)
        fail("dc_restore state", case_no, ticks, fe[FE_DC_STATE], dc);
    for (int i = 0;  i < kHdlcRxWords;  i++)
    {
        const int want = next_int();
        if (w[i] != want)
            fail("a framer word", case_no, i, w[i], want);
    }
    for (int i = 0;  i < kHdlcBuf;  i++)
    {
        const int want = next_int();
        const int got = (int) ((frame[i >> 2] >> (8*(i & 3))) & 0xFFu);
        if (got != want)
            fail("a buffer octet", case_no, i, got, want);
    }
    return checked + 1 + kHdlcRxWords + kHdlcBuf;
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: faxfe_host <cases file>\n");
        return 2;
    }
    int cases = 0;
    long long checked = 0;
    for (;;)
    {
        char tag[8];
        if (fscanf(in, "%7s", tag) != 1)
        {
            fprintf(stderr, "cases file cut short\n");
            return 2;
        }
        if (tag[0] == 'E')
            break;
        if (tag[0] != 'C')
        {
            fprintf(stderr, "unknown record %s\n", tag);
            return 2;
        }
        checked += one_case(cases);
        cases++;
    }
    fclose(in);
    printf("ok %d cases, %lld values equal to the reference's\n", cases, checked);
    return 0;
}
