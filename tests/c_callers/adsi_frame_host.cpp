// adsi_frame_host.cpp -- the message framers of the caller-ID banks (spandsp_amd/csrc/adsi_frame.hpp: adsi_next_bit(),
// adsi_put_bit(), adsi_put_byte(), adsi_deliver()) compiled for the host as they are, run one channel at a time beside the
// reference (oracle/_ref/libspandsp_adsi_ref.so) over a sweep file written by tests/adsi_sweep.py.  Built with the address
// and undefined-behaviour sanitizers by tests/test_adsi_sweep.py.
//
// A receiver line: the reference's adsi_rx takes the samples call by call; a second fsk_rx of the same preset records the
// bits and statuses the demodulator hands to the framer.  Those go through adsi_put_bit() call by call, and the messages of
// every call, the six framer words after every call and the message buffer at the end have to equal the reference's, every
// call within the record capacity of spangpu_adsi_rx_msg_capacity().
// A sender line: both sides are asked for bits, the reference through the get_bit its modulator has; the bits, the puts'
// returns and the ten words of the message layer after every call have to be equal.

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/adsi_frame.hpp"

extern "C" {
int glue_adsi_rx_run(int standard, const int16_t *amp, const int32_t *lens, int n_calls, uint8_t *msgs, int32_t *msg_lens,
                     int32_t *msg_calls, int room, int32_t *counts, int32_t *words, int32_t *fsk_words, uint8_t *msg, int8_t *bits,
                     int bit_room, int32_t *bit_counts);
int glue_adsi_tx_bits(int standard, const int32_t *ops, int n_ops, const uint8_t *opbytes, const int32_t *lens, int n_calls, int8_t *bits,
                      int32_t *results, int32_t *words);
}

using namespace spg;

static int capacity(int samples)
{
    return samples/120 + 1;
}

static long long g_calls, g_items;
static int g_reach[2] = {0, 1};         // the fullest record seen: count, of capacity

template <typename T> static bool take(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0  ||  fread(v.data(), sizeof(T), n, f) == n;
}

static int fail(const char *kind, int line, int call, const char *what, long long got, long long want)
{
    printf("DIFFERENT %s line %d call %d: %s is %lld, the reference has %lld\n", kind, line, call, what, got, want);
    return 1;
}

static int rx_line(FILE *f, int line)
{
    int32_t h[3];
    std::vector<int32_t> lens;
    std::vector<int16_t> amp;
    if (fread(h, sizeof(int32_t), 3, f) != 3  ||  !take(f, lens, h[1])  ||  !take(f, amp, h[2]))
        return fail("rx", line, -1, "file", 0, 1);
    const int standard = h[0];
    const int calls = h[1];
    const int room = h[2]/100 + 4;
    const int bit_room = h[2]/3 + 64;
    std::vector<uint8_t> ref_msgs((size_t) room*256);
    std::vector<int32_t> ref_lens(room), ref_calls(room), ref_counts(calls), ref_words((size_t) calls*6), bit_counts(calls);
    std::vector<int8_t> bits(bit_room);
    uint8_t ref_msg[256];
    amp.push_back(0);
    const int n = glue_adsi_rx_run(standard, amp.data(), lens.data(), calls, ref_msgs.data(), ref_lens.data(), ref_calls.data(), room,
                                   ref_counts.data(), ref_words.data(), NULL, ref_msg, bits.data(), bit_room, bit_counts.data());
    if (n < 0  ||  n > room)
        return fail("rx", line, -1, "reference run", n, 0);

    uint8_t msg[256];
    memset(msg, 0, sizeof(msg));
    AdsiRx v;
    memset(&v, 0, sizeof(v));
    v.standard = standard;
    v.msg = msg;
    int at = 0;
    int seen = 0;
    for (int k = 0;  k < calls;  k++)
    {
        const int cap = capacity(lens[k]);
        std::vector<uint8_t> rec((size_t) cap*kAdsiMsg);
        std::vector<int32_t> rec_lens(cap);
        v.rec_bytes = rec.data();
        v.rec_lens = rec_lens.data();
        v.cap = cap;
        v.count = 0;
        for (int i = 0;  i < bit_counts[k];  i++)
            adsi_put_bit(v, bits[at + i]);
        at += bit_counts[k];
        g_calls++;
        g_items += bit_counts[k];
        if (ref_counts[k] > cap)
            return fail("rx", line, k, "the capacity", cap, ref_counts[k]);
        if (v.count != ref_counts[k])
            return fail("rx", line, k, "count", v.count, ref_counts[k]);
        const long long mine = (long long) v.count*g_reach[1];
        const long long best = (long long) g_reach[0]*cap;
        if (mine > best  ||  (mine == best  &&  v.count > g_reach[0]))
        {
            g_reach[0] = v.count;
            g_reach[1] = cap;
        }
        for (int j = 0;  j < v.count;  j++, seen++)
        {
            if (ref_calls[seen] != k)
                return fail("rx", line, k, "arrival call", k, ref_calls[seen]);
            if (rec_lens[j] != ref_lens[seen])
                return fail("rx", line, k, "message length", rec_lens[j], ref_lens[seen]);
            if (memcmp(&rec[(size_t) j*kAdsiMsg], &ref_msgs[(size_t) seen*256], rec_lens[j]))
                return fail("rx", line, k, "message bytes of message", j, j);
        }
        const int32_t w[6] = {v.standard, v.ones, v.bit_pos, v.in_progress, v.msg_len, v.framing_errors};
        static const char *const names[6] = {"standard", "consecutive_ones", "bit_pos", "in_progress", "msg_len", "framing_errors"};
        for (int j = 0;  j < 6;  j++)
        {
            if (w[j] != ref_words[(size_t) k*6 + j])
                return fail("rx", line, k, names[j], w[j], ref_words[(size_t) k*6 + j]);
        }
    }
    if (memcmp(msg, ref_msg, 256))
        return fail("rx", line, calls, "msg[]", 0, 1);
    return 0;
}

static void preamble(int32_t *w, int a, int b, int c, int d)
{
    const bool jclip = (w[0] == kAdsiJclip);
    w[1] = (a < 0)  ?  (jclip  ?  0  :  300)  :  a;
    w[2] = (b < 0)  ?  (jclip  ?  75  :  80)  :  b;
    w[3] = (c < 0)  ?  5  :  c;
    w[4] = (d < 0)  ?  (jclip  ?  4  :  1)  :  d;
}

static int tx_line(FILE *f, int line)
{
    int32_t h[5];
    std::vector<int32_t> lens, ops;
    std::vector<uint8_t> blob;
    if (fread(h, sizeof(int32_t), 5, f) != 5  ||  !take(f, lens, h[1])  ||  !take(f, ops, (size_t) h[2]*6)  ||  !take(f, blob, (size_t) h[3] + 1))
        return fail("tx", line, -1, "file", 0, 1);
    const int standard = h[0];
    const int calls = h[1];
    const int n_ops = h[2];
    std::vector<int32_t> plens(h[4]);
    std::vector<uint8_t> packed((size_t) h[4]*256);
    for (int i = 0;  i < h[4];  i++)
    {
        if (fread(&plens[i], sizeof(int32_t), 1, f) != 1  ||  fread(&packed[(size_t) i*256], 1, 256, f) != 256)
            return fail("tx", line, -1, "file", 0, 1);
    }
    long long total = 0;
    for (int k = 0;  k < calls;  k++)
        total += lens[k];
    std::vector<int8_t> ref_bits(total + 1);
    std::vector<int32_t> ref_results(n_ops + 1), ref_words((size_t) calls*10);
    if (glue_adsi_tx_bits(standard, ops.data(), n_ops, blob.data(), lens.data(), calls, ref_bits.data(), ref_results.data(), ref_words.data()) != total)
        return fail("tx", line, -1, "reference run", 0, total);

    // the message layer's words (ADT_STANDARD .. ADT_TX_SIGNAL_ON) and the message, as a fresh channel of a bank has them
    int32_t w[10];
    uint8_t msg[256];
    memset(w, 0, sizeof(w));
    memset(msg, 0, sizeof(msg));
    w[0] = standard;
    preamble(w, -1, -1, -1, -1);
    w[9] = 1;
    int op = 0;
    int put = 0;
    long long at = 0;
    static const char *const names[10] = {"standard", "preamble_len", "preamble_ones_len", "postamble_ones_len", "stop_bits", "byte_no", "bit_pos",
                                          "bit_no", "msg_len", "tx_signal_on"};
    for (int k = 0;  k < calls;  k++)
    {
        for (  ;  op < n_ops  &&  ops[(size_t) op*6] <= k;  op++)
        {
            const int32_t *o = &ops[(size_t) op*6];
            if (o[1] == 1)
            {
                // adsi_put_kernel(): the busy check, the signal, the length check, the message and the bit sequencing
                int res = 1;
                const int len = plens[put];
                if (w[8] > 0)
                {
                    res = 0;
                }
                else
                {
                    w[9] = 1;
                    if (len < 0  ||  len > kAdsiMsg)
                    {
                        res = -1;
                    }
                    else
                    {
                        memcpy(msg, &packed[(size_t) put*256], len);
                        w[8] = len;
                        w[5] = w[6] = w[7] = 0;
                    }
                }
                put++;
                const int want = (ref_results[op] > 0)  ?  1  :  ref_results[op];
                if (res != want)
                    return fail("tx", line, k, "a put's return", res, want);
            }
            else if (o[1] == 2)
            {
                preamble(w, o[2], o[3], o[4], o[5]);
            }
            else if (o[1] == 4)
            {
                memset(w, 0, sizeof(w));
                memset(msg, 0, sizeof(msg));
                w[0] = standard;
                preamble(w, -1, -1, -1, -1);
                w[9] = 1;
            }
        }
        AdsiTx t;
        t.preamble_len = w[1];
        t.preamble_ones_len = w[2];
        t.postamble_ones_len = w[3];
        t.stop_bits = w[4];
        t.byte_no = w[5];
        t.bit_pos = w[6];
        t.bit_no = w[7];
        t.msg_len = w[8];
        t.signal_on = w[9];
        t.msg = msg;
        for (int i = 0;  i < lens[k];  i++)
        {
            int bit = adsi_next_bit(t);
            bit = (bit == -1)  ?  -7  :  bit;       // SIG_STATUS_END_OF_DATA
            if (bit != ref_bits[at + i])
                return fail("tx", line, k, "a bit", bit, ref_bits[at + i]);
        }
        at += lens[k];
        g_calls++;
        g_items += lens[k];
        w[5] = t.byte_no;
        w[6] = t.bit_pos;
        w[7] = t.bit_no;
        w[8] = t.msg_len;
        w[9] = t.signal_on;
        for (int j = 0;  j < 10;  j++)
        {
            if (w[j] != ref_words[(size_t) k*10 + j])
                return fail("tx", line, k, names[j], w[j], ref_words[(size_t) k*10 + j]);
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2)
    {
        fprintf(stderr, "usage: %s sweep-file\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    int32_t h[3];
    if (f == NULL  ||  fread(h, sizeof(int32_t), 3, f) != 3  ||  h[0] != 0x41445349)
    {
        fprintf(stderr, "%s is not a sweep file\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (int i = 0;  i < h[1];  i++)
        bad += rx_line(f, i);
    printf("rx: %d lines, %lld calls, %lld items\n", h[1], g_calls, g_items);
    printf("fullest record: %d of %d\n", g_reach[0], g_reach[1]);
    g_calls = g_items = 0;
    for (int i = 0;  i < h[2];  i++)
        bad += tx_line(f, i);
    printf("tx: %d lines, %lld calls, %lld items\n", h[2], g_calls, g_items);
    fclose(f);
    if (bad)
    {
        printf("FAILED %d lines\n", bad);
        return 1;
    }
    printf("ok %d lines\n", h[1] + h[2]);
    return 0;
}
