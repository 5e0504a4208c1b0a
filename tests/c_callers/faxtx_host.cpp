// faxtx_host.cpp -- the per-channel step functions of spandsp_amd/csrc/faxtx_dev.hpp, and hdlc_tx_get_bit() of hdlc_dev.hpp as
// the senders' bit source, compiled for the host and run one lane at a time over every tick of every case of
// tests/golden/faxtx.npz (tests/test_faxtx.py writes the cases out as whitespace separated integers and builds this file with
// -fsanitize=address,undefined).  The recorded (offered, returned) of the reference's handler calls stand in for the senders.
// Exit status 0 and "ok ..." on the last line: every span, handler, transmit word, length, step and underflow count, every bit
// a sender was answered with and the final words equal the reference's.
//
//   faxtx_host <cases file>
//
// The file: records that start with a letter.
//   C use_tep ticks samples n_frames n_ops
//     n_frames x: len octets..
//     n_ops x: tick op a b c d path
//     ticks x: len steps underflows handler transmit, n_calls x (which offered returned), n_asked answers..
//     silence remaining, total, current_tx_type, fast_modem, 16 hdlc_tx words, 404 buffer octets
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/faxtx_dev.hpp"

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

enum { OP_SET = 1, OP_RESTART, OP_TEP, OP_FRAME, OP_FLAGS, OP_END, OP_BITS, OP_EOD };
static const int kDepth = 8;

struct Op
{
    int tick, op, a, b, c, d, path;
};

static void enqueue(int case_no, int tick, int32_t *w, std::vector<int32_t> &hdr, std::vector<uint32_t> &data, int kind, int arg, int corrupt,
                    const std::vector<uint8_t> *bytes)
{
    if (w[HT_Q_COUNT] >= kDepth)
        fail("queue full", case_no, tick, w[HT_Q_COUNT], kDepth);
    const int slot = (w[HT_Q_HEAD] + w[HT_Q_COUNT]) % kDepth;
    int32_t h = kind;
    if (kind == kHdlcCmdFrame)
    {
        for (int i = 0;  i < arg;  i += 4)
        {
            uint32_t v = 0;
            for (int k = 0;  k < 4  &&  i + k < arg;  k++)
                v |= (uint32_t) (*bytes)[i + k] << (8*k);
            data[(size_t) slot*kHdlcBufWords + (i >> 2)] = v;
        }
        h |= (corrupt  ?  kHdlcCmdCorrupt  :  0) | (arg << 8);
    }
    else if (kind == kHdlcCmdFlags)
        h |= (int32_t) ((uint32_t) arg << 8);
    hdr[slot] = h;
    w[HT_Q_COUNT]++;
}

static long long run_case(int case_no, long long *bits_checked)
{
    const int use_tep = next_int();
    const int ticks = next_int();
    const int samples = next_int();
    const int n_frames = next_int();
    const int n_ops = next_int();
    std::vector<std::vector<uint8_t>> frames(n_frames);
    for (auto &f : frames)
    {
        f.resize(next_int());
        for (auto &o : f)
            o = (uint8_t) next_int();
    }
    std::vector<Op> ops(n_ops);
    for (Op &o : ops)
    {
        o.tick = next_int(); o.op = next_int(); o.a = next_int(); o.b = next_int(); o.c = next_int(); o.d = next_int(); o.path = next_int();
    }
    int32_t fx[kFaxTxWords];
    faxtx_words_init(fx, use_tep);
    int32_t w[kHdlcTxWords];
    hdlc_tx_words_init(w, 0, 2);
    // exactly the buffer's and the queue's sizes: a step outside them is the sanitizer's to find
    std::vector<uint32_t> frame(kHdlcBufWords, 0);
    std::vector<int32_t> hdr(kDepth, 0);
    std::vector<uint32_t> data((size_t) kDepth*kHdlcBufWords, 0);
    long long calls_checked = 0;
    for (int t = 0;  t < ticks;  t++)
    {
        for (const Op &o : ops)
        {
            if (o.tick != t)
                continue;
            switch (o.op)
            {
            case OP_SET:
            {
                FaxTxAct act;
                faxtx_set_tx_type(fx, o.a, o.b, o.c, o.d, &act);
                const int path = !act.acted  ?  0  :  !act.fast  ?  1  :  act.fast_init  ?  2  :  3;
                if (path != o.path)
                    fail("what set_tx_type did", case_no, t, path, o.path);
                if (act.flags)
                    hdlc_tx_flags_now(w, act.flags);
                break;
            }
            case OP_RESTART:
                fx[FX_CURRENT_TX_TYPE] = -1;
                break;
            case OP_TEP:
                fx[FX_USE_TEP] = o.a  ?  1  :  0;
                break;
            case OP_FRAME:
                enqueue(case_no, t, w, hdr, data, kHdlcCmdFrame, (int) frames[o.a].size(), o.b, &frames[o.a]);
                break;
            case OP_FLAGS:
                enqueue(case_no, t, w, hdr, data, kHdlcCmdFlags, o.a, 0, NULL);
                break;
            case OP_END:
                enqueue(case_no, t, w, hdr, data, kHdlcCmdEnd, 0, 0, NULL);
                break;
            }
        }
        const int ref_len = next_int();
        const int ref_steps = next_int();
        const int ref_under = next_int();
        const int ref_handler = next_int();
        const int ref_transmit = next_int();
        const int n_calls = next_int();
        // the reference's calls of the tick: silence calls, then at most one sender's
        int silence = 0;
        int which = -1;
        int offered = 0;
        int returned = 0;
        for (int k = 0;  k < n_calls;  k++)
        {
            const int wh = next_int();
            const int off = next_int();
            const int ret = next_int();
            if (wh == kFaxTxSilence  &&  which < 0)
                silence += ret;
            else if (which < 0)
            {
                which = wh;
                offered = off;
                returned = ret;
            }
            else
                fail("more than one sender call in a tick", case_no, t, wh, -1);
        }
        int32_t span[kSpanRows];
        faxtx_plan(fx, samples, span);
        if (span[SPAN_START] != silence)
            fail("where the silence ends", case_no, t, span[SPAN_START], silence);
        if (span[SPAN_COUNT] != ((which < 0)  ?  0  :  offered))
            fail("what the sender is offered", case_no, t, span[SPAN_COUNT], offered);
        if (which >= 0  &&  fx[FX_HANDLER] != which)
            fail("the sender", case_no, t, fx[FX_HANDLER], which);
        if (span[SPAN_START] < 0  ||  span[SPAN_START] + span[SPAN_COUNT] > samples)
            fail("a span outside the row", case_no, t, span[SPAN_START] + span[SPAN_COUNT], samples);
        // the sender's bits
        const int n_asked = next_int();
        int calls = 0;
        int empty = 0;
        const bool framed = (which == kFaxTxV21)  ||  (which == kFaxTxFast  &&  fx[FX_HDLC_MODE]);
        if (!framed  &&  n_asked)
            fail("bits asked of the framer by a sender that has another source", case_no, t, 0, n_asked);
        if (framed)
        {
            HdlcBuf buf;
            buf.open(frame.data(), 1);
            HdlcTxQueue q;
            q.hdr = hdr.data();
            q.data = data.data();
            q.depth = kDepth;
            q.underflows = 0;
            hdlc_tx_offer(w, buf, q);
            for (int i = 0;  i < n_asked;  i++)
            {
                const int ref = next_int();
                const int bit = hdlc_tx_get_bit(w, buf, q);
                if (bit != ref)
                    fail("a bit", case_no, t, bit, ref);
            }
            buf.close();
            calls = q.calls;
            empty = q.underflows;
            *bits_checked += n_asked;
        }
        int32_t out[kFaxTxOutRows];
        int lo;
        int hi;
        faxtx_resolve(fx, samples, span, returned, calls, empty, out, &lo, &hi);
        if (out[FXO_LEN] != ref_len)
            fail("len", case_no, t, out[FXO_LEN], ref_len);
        if (out[FXO_STEPS] != ref_steps)
            fail("steps", case_no, t, out[FXO_STEPS], ref_steps);
        if (out[FXO_UNDERFLOWS] != ref_under)
            fail("underflows", case_no, t, out[FXO_UNDERFLOWS], ref_under);
        if (out[FXO_HANDLER] != ref_handler)
            fail("handler", case_no, t, out[FXO_HANDLER], ref_handler);
        if (out[FXO_TRANSMIT] != ref_transmit)
            fail("transmit", case_no, t, out[FXO_TRANSMIT], ref_transmit);
        if (lo < 0  ||  hi > samples  ||  lo > hi)
            fail("what the sender wrote", case_no, t, hi, samples);
        calls_checked += n_calls;
    }
    const int ref_end[4] = {next_int(), next_int(), next_int(), next_int()};
    const int got_end[4] = {fx[FX_SIL_REMAINING], fx[FX_SIL_TOTAL], fx[FX_CURRENT_TX_TYPE], fx[FX_FAST_MODEM]};
    for (int i = 0;  i < 4;  i++)
    {
        if (got_end[i] != ref_end[i])
            fail("a final word", case_no, i, got_end[i], ref_end[i]);
    }
    for (int i = 0;  i < kHdlcTxRefWords;  i++)
    {
        const int r = next_int();
        if (w[i] != r)
            fail("a final hdlc_tx word", case_no, i, w[i], r);
    }
    for (int i = 0;  i < kHdlcBuf;  i++)
    {
        const int r = next_int();
        const int got = (int) ((frame[i >> 2] >> (8*(i & 3))) & 0xFF);
        if (got != r)
            fail("a buffer octet", case_no, i, got, r);
    }
    return calls_checked;
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: faxtx_host <cases file>\n");
        return 2;
    }
    int cases = 0;
    long long calls = 0;
    long long bits = 0;
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
        if (tag[0] != 'C')
        {
            fprintf(stderr, "unknown record %s\n", tag);
            return 2;
        }
        calls += run_case(cases++, &bits);
    }
    fclose(in);
    printf("ok %d cases, %lld handler calls, %lld bits\n", cases, calls, bits);
    return 0;
}
