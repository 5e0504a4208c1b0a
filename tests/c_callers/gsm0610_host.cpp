// gsm0610_host.cpp -- the per-frame functions of spandsp_amd/csrc/gsm0610_dev.hpp compiled for the host and run one lane at a
// time over every case of tests/golden/gsm0610.npz (tests/test_gsm0610.py writes the cases out as whitespace separated
// integers and builds this file with -fsanitize=address,undefined).  Exit status 0 and "ok ..." on the last line: every code
// byte, sample, count and state word equals the reference's after every call of the fixture's schedule; the same streams
// cut into calls of one unit each give the same output and the same final state; and every call made exactly what the
// capacity functions say.
//
//   gsm0610_host <cases file>
//
// The file: records that start with a letter.
//   C kind packing n_in n_out n_calls              kind 0: encode (in: samples, out: bytes), 1: decode (in: bytes, out: samples)
//     n_in inputs, n_out outputs
//     n_calls x: len count, 160 words: the state words after the call
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/gsm0610_dev.hpp"

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

static void fail(const char *what, int case_no, int call, long long at, long long got, long long want)
{
    fprintf(stderr, "case %d call %d: %s %lld: got %lld, reference %lld\n", case_no, call, what, at, got, want);
    exit(1);
}

struct Call
{
    int len, count;
    int32_t words[kGsmWords];
};

struct ByteSink
{
    std::vector<int32_t> *out;
    void word(uint32_t w)
    {
        for (int i = 0;  i < 4;  i++)
            out->push_back((int32_t) ((w >> (8*i)) & 0xFF));
    }
};

// one call of one channel, as a lane of the kernels makes it: from the words and back to them
static int encode_call(int32_t *w, const int32_t *row, int n, std::vector<int32_t> &out)
{
    Gsm s;
    GsmHostMem m;
    memset(&m, 0, sizeof(m));
    gsm_load(s, w, 1);
    gsm_load_hist(m, w, 1);
    const size_t before = out.size();
    ByteSink sink = {&out};
    GsmBitsOut bits;
    gsm_bits_begin(bits, s.packing);
    for (int f = 0;  f < n/kGsmFrame;  f++)
    {
        for (int k = 0;  k < kGsmFrame;  k++)
            m.st(kGsmHist + k, gsm_preprocess(s, row[f*kGsmFrame + k] & 0xFFFF));
        gsm_encode_frame(s, m, bits, sink);
    }
    gsm_bits_end(bits, sink);
    // (the last word carries zeros past the count, as the last chunk of a row does)
    const int made = (int) gsm0610_encode_capacity(s.packing, n);
    if ((int) (out.size() - before) < made)
        fail("the stream is shorter than the count", -1, -1, n, (long long) (out.size() - before), made);
    for (size_t i = before + made;  i < out.size();  i++)
    {
        if (out[i] != 0)
            fail("bits past the count", -1, -1, (long long) i, out[i], 0);
    }
    out.resize(before + made);
    gsm_store(s, w, 1);
    gsm_store_hist(m, w, 1);
    return made;
}

static int decode_call(int32_t *w, const int32_t *bytes, int n, std::vector<int32_t> &out)
{
    Gsm s;
    GsmHostMem m;
    memset(&m, 0, sizeof(m));
    gsm_load(s, w, 1);
    gsm_load_hist(m, w, 1);
    const int frames = (int) (gsm0610_decode_capacity(s.packing, n)/kGsmFrame);
    for (int f = 0;  f < frames;  f++)
    {
        const int start = (s.packing == kGsmWav49)  ?  ((f >> 1)*520 + (f & 1)*260)  :  (f*8*gsm0610_unit_bytes(s.packing));
        const int byte0 = start >> 3;
        // the stage starts at the 32-bit word of the row that holds the frame's first byte, as in the kernel
        const int from = byte0 & ~3;
        for (int i = 0;  i < kGsmStageBytes;  i++)
            m.stage_byte(i, (uint8_t) ((from + i < n)  ?  bytes[from + i]  :  0xFF));
        int32_t LARc[8], cur[8], prev[8], rrp[8];
        gsm_decode_residual(s, m, 8*(byte0 & 3) + (start & 7), LARc);
        gsm_decode_lar(s, LARc, cur, prev);
        for (int range = 0;  range < 4;  range++)
        {
            gsm_range_rp(range, cur, prev, rrp);
            for (int k = gsm_range_start(range);  k < gsm_range_start(range + 1);  k++)
                out.push_back(gsm_decode_sample(s, m, k, rrp));
        }
        gsm_shift_hist(m);
    }
    gsm_store(s, w, 1);
    gsm_store_hist(m, w, 1);
    return frames*kGsmFrame;
}

static long long reached[2];

static int run_call(int kind, int32_t *w, const int32_t *data, int n, std::vector<int32_t> &out, int case_no, int call)
{
    const int packing = w[GW_PACKING];
    const int made = kind  ?  decode_call(w, data, n, out)  :  encode_call(w, data, n, out);
    const long long cap = kind  ?  gsm0610_decode_capacity(packing, n)  :  gsm0610_encode_capacity(packing, n);
    if (made > cap)
        fail("capacity passed, len", case_no, call, n, made, cap);
    if (made == cap)
        reached[kind]++;
    return made;
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: gsm0610_host <cases file>\n");
        return 2;
    }
    int n_cases = 0;
    long long n_items = 0;
    for (;;)
    {
        char tag[8];
        if (fscanf(in, "%7s", tag) != 1  ||  tag[0] == 'E')
            break;
        const int kind = next_int();
        const int packing = next_int();
        const int n_in = next_int();
        const int n_out = next_int();
        const int n_calls = next_int();
        std::vector<int32_t> data(n_in), want(n_out);
        for (int i = 0;  i < n_in;  i++)
            data[i] = next_int();
        for (int i = 0;  i < n_out;  i++)
            want[i] = next_int();
        std::vector<Call> calls(n_calls);
        for (Call &c : calls)
        {
            c.len = next_int();
            c.count = next_int();
            for (int w = 0;  w < kGsmWords;  w++)
                c.words[w] = next_int();
        }
        if (n_calls == 0)
            fail("no calls in the case", n_cases, n_calls, 0, 0, 1);
        int32_t w[kGsmWords];
        if (!gsm0610_init_words(w, packing))
            fail("the packing is refused", n_cases, 0, 0, packing, 0);
        // ---- the fixture's schedule: every call against the reference ----
        std::vector<int32_t> got;
        int at = 0;
        for (int k = 0;  k < n_calls;  k++)
        {
            const size_t before = got.size();
            const int made = run_call(kind, w, data.data() + at, calls[k].len, got, n_cases, k);
            at += calls[k].len;
            if (made != calls[k].count)
                fail("count of call", n_cases, k, k, made, calls[k].count);
            for (size_t i = before;  i < got.size();  i++)
            {
                if (i >= want.size()  ||  got[i] != want[i])
                    fail("output", n_cases, k, (long long) i, got[i], (i < want.size())  ?  want[i]  :  -1);
            }
            for (int i = 0;  i < kGsmWords;  i++)
            {
                if (w[i] != calls[k].words[i])
                    fail("state word", n_cases, k, i, w[i], calls[k].words[i]);
            }
        }
        if (at != n_in  ||  got.size() != want.size())
            fail("items", n_cases, n_calls, at, (long long) got.size(), (long long) want.size());
        // ---- another cut of the same stream: a unit a call ----
        (void) gsm0610_init_words(w, packing);
        std::vector<int32_t> again;
        const int unit = kind  ?  gsm0610_unit_bytes(packing)  :  gsm0610_unit_samples(packing);
        for (at = 0;  at < n_in;  at += unit)
            (void) run_call(kind, w, data.data() + at, unit, again, n_cases, -1);
        if (again != got)
            fail("the second schedule's output differs, items", n_cases, -1, 0, (long long) again.size(), (long long) got.size());
        for (int i = 0;  i < kGsmWords;  i++)
        {
            if (w[i] != calls[n_calls - 1].words[i])
                fail("state word after the second schedule", n_cases, -1, i, w[i], calls[n_calls - 1].words[i]);
        }
        n_items += n_in;
        n_cases++;
    }
    fclose(in);
    if (reached[0] == 0  ||  reached[1] == 0)
    {
        fprintf(stderr, "no call reached its capacity: encode %lld, decode %lld\n", reached[0], reached[1]);
        return 1;
    }
    printf("capacity reached: encode %lld, decode %lld calls\n", reached[0], reached[1]);
    printf("ok %d cases, %lld items\n", n_cases, n_items);
    return 0;
}
