// hdlc_host.cpp -- the per-channel step functions of spandsp_amd/csrc/hdlc_dev.hpp compiled for the host and run one lane at
// a time over every sender and receiver case of tests/golden/hdlc.npz (tests/test_hdlc.py writes the cases out as whitespace
// separated integers and builds this file with -fsanitize=address,undefined), then over the streams the capacity function
// is derived from.  Exit status 0 and "ok ..." on the last line: every bit, record, octet, statistic and state word equals
// the reference's, and no stream reached its capacity's end.
//
//   hdlc_host <cases file>
//
// The file: records that start with a letter.
//   T crc32 iff depth calls n_ops
//     n_ops x: call command argument corrupt result, then for a FRAME its `argument` octets
//     calls x: want len underflows ended, 16 state words, len bits
//   R form crc32 report_bad threshold max_len interval calls n_midops           form 0: events, 1: octets
//     n_midops x: call len
//     calls x: n entries.., n_recs records.., 18 state words
//     n_bytes octets.., 404 buffer octets
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/hdlc_dev.hpp"

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

static void fail(const char *what, int case_no, int call, long long got, long long want)
{
    fprintf(stderr, "case %d call %d: %s: got %lld, reference %lld\n", case_no, call, what, got, want);
    exit(1);
}

struct Op
{
    int call, kind, arg, corrupt, result;
    std::vector<uint8_t> bytes;
};

// the host side of a channel's queue, as hdlc_tx_enqueue_kernel keeps it
static int offer(int32_t *w, std::vector<int32_t> &hdr, std::vector<uint32_t> &data, int depth, const Op &op)
{
    if (w[HT_Q_COUNT] >= depth  ||  (op.kind == kHdlcCmdFrame  &&  op.arg > w[HT_MAX_FRAME_LEN]))
        return -1;
    const int slot = (w[HT_Q_HEAD] + w[HT_Q_COUNT]) % depth;
    int32_t h = op.kind;
    if (op.kind == kHdlcCmdFrame)
    {
        for (int i = 0;  i < op.arg;  i += 4)
        {
            uint32_t v = 0;
            for (int k = 0;  k < 4  &&  i + k < op.arg;  k++)
                v |= (uint32_t) op.bytes[i + k] << (8*k);
            data[(size_t) slot*kHdlcBufWords + (i >> 2)] = v;
        }
        h |= (op.corrupt  ?  kHdlcCmdCorrupt  :  0) | (op.arg << 8);
    }
    else if (op.kind == kHdlcCmdFlags)
        h |= (int32_t) ((uint32_t) op.arg << 8);
    hdr[slot] = h;
    w[HT_Q_COUNT]++;
    return 0;
}

static long long tx_case(int case_no)
{
    const int crc32 = next_int();
    const int iff = next_int();
    const int depth = next_int();
    const int calls = next_int();
    const int n_ops = next_int();
    std::vector<Op> ops(n_ops);
    for (Op &op : ops)
    {
        op.call = next_int();
        op.kind = next_int();
        op.arg = next_int();
        op.corrupt = next_int();
        op.result = next_int();
        if (op.kind == kHdlcCmdFrame)
        {
            op.bytes.resize(op.arg);
            for (int i = 0;  i < op.arg;  i++)
                op.bytes[i] = (uint8_t) next_int();
        }
    }
    int32_t w[kHdlcTxWords];
    hdlc_tx_words_init(w, crc32, iff);
    // exactly the buffer's and the queue's sizes: a step outside them is the sanitizer's to find
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    std::vector<int32_t> hdr(depth, 0);
    std::vector<uint32_t> data((size_t) depth*kHdlcBufWords, 0);
    long long checked = 0;
    for (int k = 0;  k < calls;  k++)
    {
        for (const Op &op : ops)
        {
            if (op.call == k)
            {
                const int r = offer(w, hdr, data, depth, op);
                if (r != op.result)
                    fail("result of a command", case_no, k, r, op.result);
            }
        }
        const int want = next_int();
        const int len = next_int();
        const int under = next_int();
        const int ended = next_int();
        int32_t ref_words[kHdlcTxRefWords];
        for (int i = 0;  i < kHdlcTxRefWords;  i++)
            ref_words[i] = next_int();
        std::vector<uint8_t> bits((want + 7)/8, 0);
        HdlcBuf buf;
        buf.open(frame.data(), 1);
        HdlcTxQueue q;
        q.hdr = hdr.data();
        q.data = data.data();
        q.depth = depth;
        q.underflows = 0;
        int got_ended = 0;
        const int got = hdlc_tx_run(w, buf, q, bits.data(), want, &got_ended);
        buf.close();
        if (got != len)
            fail("bits produced", case_no, k, got, len);
        if (got_ended != ended)
            fail("end of data", case_no, k, got_ended, ended);
        if (q.underflows != under)
            fail("underflows", case_no, k, q.underflows, under);
        for (int i = 0;  i < len;  i++)
        {
            const int bit = next_int();
            if (((bits[i >> 3] >> (i & 7)) & 1) != bit)
                fail("a bit", case_no, k, i, bit);
        }
        for (int i = 0;  i < kHdlcTxRefWords;  i++)
        {
            if (w[i] != ref_words[i])
                fail("a state word", case_no, k, w[i], ref_words[i]);
        }
        checked += len;
    }
    return checked;
}

static long long rx_case(int case_no)
{
    const int form = next_int();
    const int crc32 = next_int();
    const int bad = next_int();
    const int thr = next_int();
    const int max_len = next_int();
    const int interval = next_int();
    const int calls = next_int();
    const int n_midops = next_int();
    std::vector<int> mid(2*n_midops);
    for (int &v : mid)
        v = next_int();
    int32_t w[kHdlcRxWords];
    hdlc_rx_words_init(w, crc32, bad, thr);
    if (max_len >= 0)
        w[HR_MAX_FRAME_LEN] = (max_len + w[HR_CRC_BYTES] <= kHdlcBuf)  ?  (max_len + w[HR_CRC_BYTES])  :  kHdlcBuf;
    w[HR_OCTET_COUNT_REPORT_INTERVAL] = interval;
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    std::vector<uint8_t> all_bytes;
    long long checked = 0;
    for (int k = 0;  k < calls;  k++)
    {
        for (int i = 0;  i < n_midops;  i++)
        {
            if (mid[2*i] == k)
                w[HR_MAX_FRAME_LEN] = (mid[2*i + 1] + w[HR_CRC_BYTES] <= kHdlcBuf)  ?  (mid[2*i + 1] + w[HR_CRC_BYTES])  :  kHdlcBuf;
        }
        const int n = next_int();
        std::vector<int> entries(n);
        for (int &v : entries)
            v = next_int();
        long long rec_cap;
        long long byte_cap;
        hdlc_rx_capacity(form  ?  8LL*n  :  n, &rec_cap, &byte_cap);
        std::vector<int32_t> recs(rec_cap);
        std::vector<uint8_t> bytes(byte_cap);
        HdlcRxSink out;
        out.recs = recs.data();
        out.bytes = bytes.data();
        out.rec_cap = (int) rec_cap;
        out.byte_cap = (int) byte_cap;
        out.n_recs = 0;
        out.n_bytes = 0;
        HdlcBuf buf;
        buf.open(frame.data(), 1);
        for (int e : entries)
        {
            if (form)
                hdlc_rx_octet(w, buf, out, e);
            else
                hdlc_rx_event(w, buf, out, e);
        }
        buf.close();
        if (out.n_recs > rec_cap  ||  out.n_bytes > byte_cap)
            fail("capacity", case_no, k, out.n_recs, rec_cap);
        const int n_recs = next_int();
        if (out.n_recs != n_recs)
            fail("records", case_no, k, out.n_recs, n_recs);
        for (int i = 0;  i < n_recs;  i++)
        {
            const int r = next_int();
            if (recs[i] != r)
                fail("a record", case_no, k, recs[i], r);
        }
        all_bytes.insert(all_bytes.end(), bytes.begin(), bytes.begin() + out.n_bytes);
        for (int i = 0;  i < kHdlcRxWords;  i++)
        {
            const int r = next_int();
            if (w[i] != r)
                fail("a state word", case_no, k, w[i], r);
        }
        checked += n;
    }
    const int n_bytes = next_int();
    if ((int) all_bytes.size() != n_bytes)
        fail("octets delivered", case_no, calls, (long long) all_bytes.size(), n_bytes);
    for (int i = 0;  i < n_bytes;  i++)
    {
        const int r = next_int();
        if (all_bytes[i] != r)
            fail("an octet", case_no, i, all_bytes[i], r);
    }
    for (int i = 0;  i < kHdlcBuf;  i++)
    {
        const int r = next_int();
        const int got = (int) ((frame[i >> 2] >> (8*(i & 3))) & 0xFF);
        if (got != r)
            fail("a buffer octet", case_no, i, got, r);
    }
    return checked;
}

// ---- the capacity function against the streams it is derived from ------------------------------------------------------

struct Worst
{
    const char *name;
    int recs;
    int bytes;
};

// One call of `events` entries from a prepared state; what it delivered.  The sink has exactly the capacity.
static void run_worst(int32_t *w, std::vector<uint32_t> &frame, const std::vector<int> &entries, const char *name, long long *most_recs,
                      long long *most_bytes)
{
    long long rec_cap;
    long long byte_cap;
    hdlc_rx_capacity((long long) entries.size(), &rec_cap, &byte_cap);
    std::vector<int32_t> recs(rec_cap);
    std::vector<uint8_t> bytes(byte_cap);
    HdlcRxSink out;
    out.recs = recs.data();
    out.bytes = bytes.data();
    out.rec_cap = (int) rec_cap;
    out.byte_cap = (int) byte_cap;
    out.n_recs = 0;
    out.n_bytes = 0;
    HdlcBuf buf;
    buf.open(frame.data(), 1);
    for (int e : entries)
        hdlc_rx_event(w, buf, out, e);
    buf.close();
    if (out.n_recs > rec_cap  ||  out.n_bytes > byte_cap)
    {
        fprintf(stderr, "capacity: %s with %zu entries delivered %d records (%lld) and %d octets (%lld)\n", name, entries.size(), out.n_recs,
                rec_cap, out.n_bytes, byte_cap);
        exit(1);
    }
    // how close the stream comes, as parts of 1000
    if (out.n_recs*1000LL/rec_cap > *most_recs)
        *most_recs = out.n_recs*1000LL/rec_cap;
    if (out.n_bytes*1000LL/byte_cap > *most_bytes)
        *most_bytes = out.n_bytes*1000LL/byte_cap;
}

static void capacity_streams(long long *most_recs, long long *most_bytes)
{
    static const int sizes[] = {1, 2, 7, 8, 9, 15, 16, 17, 24, 192, 331, 1000, 4096};
    for (int n : sizes)
    {
        for (int crc32 = 0;  crc32 < 2;  crc32++)
        {
            int32_t w[kHdlcRxWords];
            std::vector<uint32_t> frame(kHdlcBufWords, 0xA5C3F00Fu);
            std::vector<int> e(n);
            // a run of 0x7F at report interval 1, counting already, the first abort due with the first bit
            hdlc_rx_words_init(w, crc32, 1, 1);
            w[HR_OCTET_COUNT_REPORT_INTERVAL] = 1;
            w[HR_OCTET_COUNTING_MODE] = 1;
            w[HR_RAW_BIT_STREAM] = 0x3F00;     // a zero and six ones behind the bit to come
            for (int i = 0;  i < n;  i++)
                e[i] = (i % 8 != 1);
            run_worst(w, frame, e, "aborts", most_recs, most_bytes);
            // a bad one-octet frame every 16 bits
            hdlc_rx_words_init(w, crc32, 1, 1);
            w[HR_FLAGS_SEEN] = 1;
            w[HR_FRAMING_OK_ANNOUNCED] = 1;
            for (int i = 0;  i < n;  i++)
                e[i] = (i % 16 < 8)  ?  ((0xA3 >> (i % 8)) & 1)  :  ((0x7E >> (i % 8)) & 1);
            run_worst(w, frame, e, "one-octet frames", most_recs, most_bytes);
            // octet reports at interval 1 on unframed bits
            hdlc_rx_words_init(w, crc32, 1, 5);
            w[HR_OCTET_COUNT_REPORT_INTERVAL] = 1;
            w[HR_OCTET_COUNTING_MODE] = 1;
            w[HR_NUM_BITS] = 7;
            for (int i = 0;  i < n;  i++)
                e[i] = (i*7 % 3 == 0);
            run_worst(w, frame, e, "octet reports", most_recs, most_bytes);
            // the longest length a channel can carry into a call, delivered by its first flag
            hdlc_rx_words_init(w, crc32, 1, 1);
            w[HR_FLAGS_SEEN] = 1;
            w[HR_FRAMING_OK_ANNOUNCED] = 1;
            w[HR_LEN] = kHdlcBuf + 1;
            w[HR_RAW_BIT_STREAM] = 0x3F00;     // a zero and six ones behind the bit to come
            for (int i = 0;  i < n;  i++)
                e[i] = (i % 16 == 0)  ?  0  :  ((i % 16 < 8)  ?  ((0x7E >> (i % 8)) & 1)  :  ((0x35 >> (i % 8)) & 1));
            run_worst(w, frame, e, "carried frame", most_recs, most_bytes);
            // nothing but reports
            hdlc_rx_words_init(w, crc32, 1, 1);
            for (int i = 0;  i < n;  i++)
                e[i] = -1 - (i % 5);
            run_worst(w, frame, e, "reports", most_recs, most_bytes);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: hdlc_host <cases file>\n");
        return 2;
    }
    int tx = 0;
    int rx = 0;
    long long bits = 0;
    long long entries = 0;
    for (;;)
    {
        char tag[8];
        if (fscanf(in, "%7s", tag) != 1)
        {
            fprintf(stderr, "no end record\n");
            return 2;
        }
        if (tag[0] == 'E')
            break;
        if (tag[0] == 'T')
            bits += tx_case(tx++);
        else if (tag[0] == 'R')
            entries += rx_case(1000 + rx++);
        else
        {
            fprintf(stderr, "unknown record %s\n", tag);
            return 2;
        }
    }
    fclose(in);
    long long most_recs = 0;
    long long most_bytes = 0;
    capacity_streams(&most_recs, &most_bytes);
    printf("ok %d sender cases %lld bits, %d receiver cases %lld entries, capacity reached to %lld and %lld of 1000\n", tx, bits, rx, entries,
           most_recs, most_bytes);
    return 0;
}
