// hdlc_sweep_host.cpp -- the per-channel step functions of spandsp_amd/csrc/hdlc_dev.hpp compiled for the host and run one
// lane at a time over the generated lines of the HDLC sweep (tests/hdlc_sweep.py), beside the reference's framer run by the
// same program on the same input through the drivers of oracle/ref_glue/ref_glue_hdlc.c: tests/test_hdlc_sweep.py writes the
// lines, configurations and schedules to binary files, builds this file with -fsanitize=address,undefined and links it
// against oracle/_ref/libspandsp_hdlc_ref.so.  After every call every record, octet, count, bit and state word must be equal,
// at the end the 404 buffer octets, and every call of a receiver must stay within hdlc_rx_capacity() of its events: the
// sinks have exactly that room, so that a step past it is the sanitizer's to find as well.
// Exit status 0 and "ok ..." on the last line, or the first difference as family, configuration, line, call, item and seed.
//
//   hdlc_sweep_host <file> ...
//
// A file: int32 words, little-endian.
//   0x48444C43, records
//   a record: kind (0 a receiver's events, int16; 1 a receiver's octets; 2 a sender), line, family, five configuration words
//             (receiver: crc32, report_bad_frames, threshold, max_frame_len argument, interval; sender: crc32,
//             inter_frame_flags, queue depth, max_frame_len or -1, 0), n_calls, n_ops, n_bytes, seed, n_calls lengths (a
//             sender's wants), n_ops operations of four words (receiver: call, operation, value, 0; sender: call, command,
//             argument, corrupt), then n_bytes bytes padded to a whole word (the events or octets; a sender's frames)

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/hdlc_dev.hpp"

using namespace spg;

// the batch drivers of oracle/ref_glue/ref_glue_hdlc.c over the reference
extern "C"
{
int glue_hdlc_rx_run(int crc32, int report_bad_frames, int framing_ok_threshold, const void *events, int octets, const int32_t lens[],
                     int n_calls, const int32_t ops[], int n_ops, int32_t recs[], int rec_room, uint8_t bytes[], int byte_room,
                     int32_t n_recs[], int32_t n_bytes[], int32_t words[], const int32_t want[], uint8_t buffer[]);
int glue_hdlc_tx_run(int crc32, int inter_frame_flags, int depth, int max_frame_len, const int32_t ops[], const uint8_t opbytes[], int n_ops,
                     const int32_t wants[], int n_calls, uint8_t bits[], int32_t lens[], int32_t under[], int32_t ended[], int32_t taken[],
                     int32_t results[], int32_t words[], const int32_t want[], uint8_t buffer[]);
}

static const char *const kFamily[] = {"wire", "sent", "damaged", "noise", "ones_heavy", "abort_runs", "short_frames", "overlong", "statuses",
                                      "any_int16", "capacity"};
static const char *const kKind[] = {"receiver, events", "receiver, octets", "sender"};

struct Record
{
    int kind, line, family, cfg[5], n_calls, n_ops, seed;
    std::vector<int32_t> lens, ops;
    std::vector<uint8_t> data;
};

static void fail(const Record &r, int call, const char *what, long long at, long long got, long long want)
{
    fprintf(stderr, "%s, family %s, configuration (%d, %d, %d, %d, %d), line %d, call %d: %s %lld: got %lld, the reference has %lld (seed %#x)\n",
            kKind[r.kind], (r.kind == 2)  ?  "-"  :  kFamily[r.family], r.cfg[0], r.cfg[1], r.cfg[2], r.cfg[3], r.cfg[4], r.line, call, what, at,
            got, want, r.seed);
    exit(1);
}

static long long n_lines[3], n_calls_made[3], n_items[3], n_records, n_octets;
static long long most_recs, most_bytes;         // how close a call came to its capacities, as parts of 1000

// ---- receiver --------------------------------------------------------------------------------------------------------------

// spangpu_hdlc_rx_set_max_frame_len(), ..._set_octet_counting_report_interval() and ..._restart() on a channel's words
static void rx_control(int32_t *w, int op, int value)
{
    switch (op)
    {
    case 1:
        w[HR_MAX_FRAME_LEN] = ((long long) value + w[HR_CRC_BYTES] <= kHdlcBuf)  ?  (value + w[HR_CRC_BYTES])  :  kHdlcBuf;
        break;
    case 2:
        w[HR_OCTET_COUNT_REPORT_INTERVAL] = value;
        break;
    case 3:
        hdlc_rx_words_restart(w);
        break;
    }
}

static void run_rx(const Record &r)
{
    const bool octets = (r.kind == 1);
    long long total = 0;
    for (int k = 0;  k < r.n_calls;  k++)
        total += r.lens[k];
    const long long bits = total*(octets  ?  8  :  1);
    std::vector<int32_t> ops3;
    for (int i = 0;  i < r.n_ops;  i++)
        ops3.insert(ops3.end(), r.ops.begin() + 4*i, r.ops.begin() + 4*i + 3);
    // the reference: the whole line, with the words after every call
    std::vector<int32_t> ref_recs((size_t) (2*bits + 2*r.n_calls + 8));
    std::vector<uint8_t> ref_bytes((size_t) (bits/8 + 404LL*r.n_calls + 8));
    std::vector<int32_t> ref_nrecs(r.n_calls), ref_nbytes(r.n_calls), ref_words((size_t) r.n_calls*kHdlcRxWords), want(r.n_calls, 1);
    uint8_t ref_buffer[kHdlcBuf];
    // (a copy of exactly the line's size, so that the sanitizer sees a read past it)
    std::vector<uint8_t> events(r.data.begin(), r.data.end());
    const int rc = glue_hdlc_rx_run(r.cfg[0], r.cfg[1], r.cfg[2], events.data(), octets, r.lens.data(), r.n_calls, ops3.data(), r.n_ops, ref_recs.data(),
                                    (int) ref_recs.size(), ref_bytes.data(), (int) ref_bytes.size(), ref_nrecs.data(), ref_nbytes.data(),
                                    ref_words.data(), want.data(), ref_buffer);
    if (rc < 0)
        fail(r, -1, "the reference's driver refused the line, code", 0, rc, 0);
    // the step functions: one channel's words, its buffer of exactly 101 words
    int32_t w[kHdlcRxWords];
    hdlc_rx_words_init(w, r.cfg[0], r.cfg[1], r.cfg[2]);
    for (int i = 0;  i < r.n_ops;  i++)
    {
        if (r.ops[4*i] < 0)
            rx_control(w, r.ops[4*i + 1], r.ops[4*i + 2]);
    }
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    size_t at = 0, rec_at = 0, byte_at = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        const int n = r.lens[k];
        long long rec_cap = 0, byte_cap = 0;
        HdlcRxSink out;
        std::vector<int32_t> recs;
        std::vector<uint8_t> bytes;
        out.recs = NULL;
        out.bytes = NULL;
        out.rec_cap = 0;
        out.byte_cap = 0;
        out.n_recs = 0;
        out.n_bytes = 0;
        if (n > 0)
        {
            for (int i = 0;  i < r.n_ops;  i++)
            {
                if (r.ops[4*i] == k)
                    rx_control(w, r.ops[4*i + 1], r.ops[4*i + 2]);
            }
            hdlc_rx_capacity(octets  ?  8LL*n  :  n, &rec_cap, &byte_cap);
            recs.resize((size_t) rec_cap);
            bytes.resize((size_t) byte_cap);
            out.recs = recs.data();
            out.bytes = bytes.data();
            out.rec_cap = (int) rec_cap;
            out.byte_cap = (int) byte_cap;
            HdlcBuf buf;
            buf.open(frame.data(), 1);
            if (octets)
            {
                for (int i = 0;  i < n;  i++)
                    hdlc_rx_octet(w, buf, out, events[at + i]);
            }
            else
            {
                for (int i = 0;  i < n;  i++)
                    hdlc_rx_event(w, buf, out, (int16_t) (events[2*(at + i)] | (events[2*(at + i) + 1] << 8)));
            }
            buf.close();
            at += (size_t) n;
            // the reference's own counts against the capacities, then ours against the reference's
            if (ref_nrecs[k] > rec_cap)
                fail(r, k, "the record capacity is passed by the reference, events", n, ref_nrecs[k], rec_cap);
            if (ref_nbytes[k] > byte_cap)
                fail(r, k, "the octet capacity is passed by the reference, events", n, ref_nbytes[k], byte_cap);
            if (ref_nrecs[k]*1000LL/rec_cap > most_recs)
                most_recs = ref_nrecs[k]*1000LL/rec_cap;
            if (ref_nbytes[k]*1000LL/byte_cap > most_bytes)
                most_bytes = ref_nbytes[k]*1000LL/byte_cap;
            n_calls_made[r.kind]++;
            n_items[r.kind] += n;
        }
        if (out.n_recs != ref_nrecs[k])
            fail(r, k, "records of call", k, out.n_recs, ref_nrecs[k]);
        for (int i = 0;  i < out.n_recs;  i++)
        {
            if (recs[i] != ref_recs[rec_at + i])
                fail(r, k, "record", i, recs[i], ref_recs[rec_at + i]);
        }
        if (out.n_bytes != ref_nbytes[k])
            fail(r, k, "octets of call", k, out.n_bytes, ref_nbytes[k]);
        for (int i = 0;  i < out.n_bytes;  i++)
        {
            if (bytes[i] != ref_bytes[byte_at + i])
                fail(r, k, "octet", i, bytes[i], ref_bytes[byte_at + i]);
        }
        rec_at += (size_t) out.n_recs;
        byte_at += (size_t) out.n_bytes;
        for (int i = 0;  i < kHdlcRxWords;  i++)
        {
            if (w[i] != ref_words[(size_t) k*kHdlcRxWords + i])
                fail(r, k, "state word", i, w[i], ref_words[(size_t) k*kHdlcRxWords + i]);
        }
    }
    for (int i = 0;  i < kHdlcBuf;  i++)
    {
        const int got = (int) ((frame[i >> 2] >> (8*(i & 3))) & 0xFF);
        if (got != ref_buffer[i])
            fail(r, r.n_calls, "buffer octet", i, got, ref_buffer[i]);
    }
    n_records += (long long) rec_at;
    n_octets += (long long) byte_at;
}

// ---- sender ----------------------------------------------------------------------------------------------------------------

// the host side of a channel's queue, as hdlc_tx_enqueue_kernel keeps it
static int offer(int32_t *w, std::vector<int32_t> &hdr, std::vector<uint32_t> &data, int depth, int kind, int arg, int corrupt, const uint8_t *bytes)
{
    if (w[HT_Q_COUNT] >= depth  ||  (kind == kHdlcCmdFrame  &&  arg > w[HT_MAX_FRAME_LEN]))
        return -1;
    int slot = w[HT_Q_HEAD] + w[HT_Q_COUNT];
    slot -= (slot >= depth)  ?  depth  :  0;
    int32_t h = kind;
    if (kind == kHdlcCmdFrame)
    {
        if (arg == 0)
            h = kHdlcCmdEnd;
        else
        {
            for (int i = 0;  i < arg;  i += 4)
            {
                uint32_t v = 0;
                for (int k = 0;  k < 4  &&  i + k < arg;  k++)
                    v |= (uint32_t) bytes[i + k] << (8*k);
                data[(size_t) slot*kHdlcBufWords + (i >> 2)] = v;
            }
            h = kHdlcCmdFrame | (corrupt  ?  kHdlcCmdCorrupt  :  0) | (arg << 8);
        }
    }
    else if (kind == kHdlcCmdFlags)
        h = kHdlcCmdFlags | (int32_t) ((uint32_t) arg << 8);
    hdr[slot] = h;
    w[HT_Q_COUNT]++;
    return 0;
}

static void run_tx(const Record &r)
{
    const int depth = r.cfg[2];
    long long total = 0;
    for (int k = 0;  k < r.n_calls;  k++)
        total += r.lens[k];
    std::vector<uint8_t> ref_bits((size_t) total + 8);
    std::vector<int32_t> ref_lens(r.n_calls), ref_under(r.n_calls), ref_ended(r.n_calls), ref_taken(r.n_calls), ref_results(r.n_ops + 1),
        ref_words((size_t) r.n_calls*kHdlcTxRefWords), want(r.n_calls, 1);
    uint8_t ref_buffer[kHdlcBuf];
    std::vector<uint8_t> opbytes(r.data.begin(), r.data.end());
    const int rc = glue_hdlc_tx_run(r.cfg[0], r.cfg[1], depth, r.cfg[3], r.ops.data(), opbytes.data(), r.n_ops, r.lens.data(), r.n_calls, ref_bits.data(),
                                    ref_lens.data(), ref_under.data(), ref_ended.data(), ref_taken.data(), ref_results.data(), ref_words.data(),
                                    want.data(), ref_buffer);
    if (rc < 0)
        fail(r, -1, "the reference's driver refused the line, code", 0, rc, 0);
    int32_t w[kHdlcTxWords];
    hdlc_tx_words_init(w, r.cfg[0], r.cfg[1]);
    if (r.cfg[3] >= 0)
        w[HT_MAX_FRAME_LEN] = (r.cfg[3] <= kHdlcMaxFrame)  ?  r.cfg[3]  :  kHdlcMaxFrame;
    // exactly the buffer's and the queue's sizes
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    std::vector<int32_t> hdr(depth, 0);
    std::vector<uint32_t> data((size_t) depth*kHdlcBufWords, 0);
    size_t byte_at = 0, bit_at = 0;
    int next_op = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        for (  ;  next_op < r.n_ops  &&  r.ops[4*next_op] <= k;  next_op++)
        {
            const int kind = r.ops[4*next_op + 1], arg = r.ops[4*next_op + 2];
            const int res = offer(w, hdr, data, depth, kind, arg, r.ops[4*next_op + 3], opbytes.data() + byte_at);
            if (kind == kHdlcCmdFrame)
                byte_at += (size_t) arg;
            if (res != ref_results[next_op])
                fail(r, k, "result of offer", next_op, res, ref_results[next_op]);
        }
        const int n = r.lens[k];
        int got = 0, ended = 0, under = 0;
        if (n > 0)
        {
            std::vector<uint8_t> bits((size_t) (n + 7)/8, 0);
            HdlcBuf buf;
            buf.open(frame.data(), 1);
            HdlcTxQueue q;
            q.hdr = hdr.data();
            q.data = data.data();
            q.depth = depth;
            q.underflows = 0;
            got = hdlc_tx_run(w, buf, q, bits.data(), n, &ended);
            buf.close();
            under = q.underflows;
            if (got != ref_lens[k])
                fail(r, k, "bits of call", k, got, ref_lens[k]);
            for (int i = 0;  i < got;  i++)
            {
                if (((bits[i >> 3] >> (i & 7)) & 1) != ref_bits[bit_at + i])
                    fail(r, k, "bit", i, (bits[i >> 3] >> (i & 7)) & 1, ref_bits[bit_at + i]);
            }
            // nothing behind the last bit in its octet
            if ((got & 7)  &&  (bits[got >> 3] >> (got & 7)))
                fail(r, k, "bits behind the last, octet", got >> 3, bits[got >> 3], 0);
            bit_at += (size_t) got;
            n_calls_made[2]++;
            n_items[2] += got;
        }
        if (got != ref_lens[k])
            fail(r, k, "bits of call", k, got, ref_lens[k]);
        if (ended != ref_ended[k])
            fail(r, k, "end of data in call", k, ended, ref_ended[k]);
        if (under != ref_under[k])
            fail(r, k, "underflows on an empty queue in call", k, under, ref_under[k]);
        for (int i = 0;  i < kHdlcTxRefWords;  i++)
        {
            if (w[i] != ref_words[(size_t) k*kHdlcTxRefWords + i])
                fail(r, k, "state word", i, w[i], ref_words[(size_t) k*kHdlcTxRefWords + i]);
        }
    }
    for (int i = 0;  i < kHdlcBuf;  i++)
    {
        const int got = (int) ((frame[i >> 2] >> (8*(i & 3))) & 0xFF);
        if (got != ref_buffer[i])
            fail(r, r.n_calls, "buffer octet", i, got, ref_buffer[i]);
    }
}

// ---- the files ------------------------------------------------------------------------------------------------------------

static int32_t next_word(FILE *in, const char *path)
{
    int32_t v;
    if (fread(&v, sizeof(v), 1, in) != 1)
    {
        fprintf(stderr, "%s: cut short\n", path);
        exit(2);
    }
    return v;
}

static void run_file(const char *path)
{
    FILE *in = fopen(path, "rb");
    if (in == NULL  ||  next_word(in, path) != 0x48444C43)
    {
        fprintf(stderr, "%s: not a sweep file\n", path);
        exit(2);
    }
    const int records = next_word(in, path);
    for (int i = 0;  i < records;  i++)
    {
        Record r;
        r.kind = next_word(in, path);
        r.line = next_word(in, path);
        r.family = next_word(in, path);
        for (int c = 0;  c < 5;  c++)
            r.cfg[c] = next_word(in, path);
        r.n_calls = next_word(in, path);
        r.n_ops = next_word(in, path);
        const int n_bytes = next_word(in, path);
        r.seed = next_word(in, path);
        if (r.kind < 0  ||  r.kind > 2  ||  r.family < 0  ||  r.family > 10  ||  r.n_calls < 1  ||  r.n_calls > 4096  ||  r.n_ops < 0
            ||  r.n_ops > 65536  ||  n_bytes < 0  ||  n_bytes > (1 << 24)  ||  (r.kind == 2  &&  (r.cfg[2] < 1  ||  r.cfg[2] > 64)))
        {
            fprintf(stderr, "%s: record %d is no record\n", path, i);
            exit(2);
        }
        r.lens.resize((size_t) r.n_calls);
        for (int32_t &v : r.lens)
            v = next_word(in, path);
        r.ops.resize((size_t) 4*r.n_ops);
        for (int32_t &v : r.ops)
            v = next_word(in, path);
        r.data.resize((size_t) (n_bytes + 3) & ~(size_t) 3);
        if (!r.data.empty()  &&  fread(r.data.data(), 1, r.data.size(), in) != r.data.size())
        {
            fprintf(stderr, "%s: cut short\n", path);
            exit(2);
        }
        r.data.resize((size_t) n_bytes);
        long long need = 0;
        if (r.kind == 2)
        {
            for (int k = 0;  k < r.n_ops;  k++)
                need += (r.ops[4*k + 1] == kHdlcCmdFrame)  ?  r.ops[4*k + 2]  :  0;
        }
        else
        {
            for (int k = 0;  k < r.n_calls;  k++)
                need += (long long) r.lens[k]*((r.kind == 0)  ?  2  :  1);
        }
        if (need != n_bytes)
        {
            fprintf(stderr, "%s: record %d: %lld bytes needed, %d bytes\n", path, i, need, n_bytes);
            exit(2);
        }
        if (r.kind == 2)
            run_tx(r);
        else
            run_rx(r);
        n_lines[r.kind]++;
    }
    fclose(in);
}

int main(int argc, char **argv)
{
    if (argc < 2)
    {
        fprintf(stderr, "usage: hdlc_sweep_host <file> ...\n");
        return 2;
    }
    for (int i = 1;  i < argc;  i++)
        run_file(argv[i]);
    printf("rx_events: %lld lines, %lld calls, %lld items\n", n_lines[0], n_calls_made[0], n_items[0]);
    printf("rx_octets: %lld lines, %lld calls, %lld items\n", n_lines[1], n_calls_made[1], n_items[1]);
    printf("tx: %lld lines, %lld calls, %lld items\n", n_lines[2], n_calls_made[2], n_items[2]);
    printf("delivered: %lld records, %lld octets; capacity reached to %lld and %lld of 1000\n", n_records, n_octets, most_recs, most_bytes);
    printf("ok %lld lines\n", n_lines[0] + n_lines[1] + n_lines[2]);
    return 0;
}
