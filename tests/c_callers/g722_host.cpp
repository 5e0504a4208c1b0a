// g722_host.cpp -- the per-code functions of spandsp_amd/csrc/g722_dev.hpp compiled for the host and run one lane at a time
// over every case of tests/golden/g722.npz (tests/test_g722.py writes the cases out as whitespace separated integers and
// builds this file with -fsanitize=address,undefined).  Exit status 0 and "ok ..." on the last line: every code, packed
// byte, sample, count and state word equals the reference's after every call of the fixture's schedule; the same streams cut
// into calls of 4, 6, 160 (encoders) or 3, 5, 160 (decoders) give the same output and the same final state; and no call
// passed the capacity functions, which some call reached.
//
//   g722_host <cases file>
//
// The file: records that start with a letter.
//   C kind rate options n_in n_out n_calls         kind 0: encode (in: samples, out: bytes), 1: decode (in: bytes, out: samples)
//     n_in inputs, n_out outputs
//     n_calls x: len count, 74 words: the state words after the call
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/g722_dev.hpp"

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
    int32_t words[kG722Words];
};

// one call of one channel, as a lane of the kernels makes it
static int encode_call(G722 &s, const int32_t *row, int n, std::vector<int32_t> &out)
{
    const int per = s.eight_k  ?  1  :  2;
    int made = 0;
    for (int i = 0;  i + per <= n;  i += per)
    {
        const int32_t code = g722_encode_code(s, kG722TabHost, row[i] & 0xFFFF, (per == 2)  ?  (row[i + 1] & 0xFFFF)  :  0);
        int32_t byte;
        if (g722_pack(s, code, &byte))
        {
            out.push_back(byte);
            made++;
        }
    }
    return made;
}

static int decode_call(G722 &s, const int32_t *bytes, int n, std::vector<int32_t> &out)
{
    if (n == 0)
        return 0;
    const int announced = g722_decode_codes(s, n);
    int codes = 0;
    int made = 0;
    for (int i = 0;  i < n;  )
    {
        int32_t byte = 0;
        if (g722_unpack_needs(s))
            byte = bytes[i++];
        const int32_t code = g722_unpack(s, byte);
        int32_t amp[2];
        g722_decode_code(s, kG722TabHost, code, amp);
        out.push_back(amp[0]);
        made++;
        if (!s.eight_k)
        {
            out.push_back(amp[1]);
            made++;
        }
        codes++;
    }
    if (codes != announced)
    {
        fprintf(stderr, "g722_decode_codes() said %d, the loop made %d\n", announced, codes);
        exit(1);
    }
    return made;
}

static long long slack[2] = {1 << 30, 1 << 30};

static int run_call(int kind, G722 &s, const int32_t *data, int n, std::vector<int32_t> &out, int case_no, int call)
{
    const int made = kind  ?  decode_call(s, data, n, out)  :  encode_call(s, data, n, out);
    const long long cap = kind  ?  g722_decode_capacity(s.bps, s.packed, s.eight_k, n)  :  g722_encode_capacity(s.bps, s.packed, s.eight_k, n);
    if (made > cap)
        fail("capacity passed, len", case_no, call, n, made, cap);
    // within one code: a byte of an encoder, a sample or a pair of a decoder
    const long long unit = (kind  &&  !s.eight_k)  ?  2  :  1;
    if ((cap - made)/unit < slack[kind])
        slack[kind] = (cap - made)/unit;
    return made;
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: g722_host <cases file>\n");
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
        const int rate = next_int();
        const int options = next_int();
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
            for (int w = 0;  w < kG722Words;  w++)
                c.words[w] = next_int();
        }
        if (n_calls == 0)
            fail("no calls in the case", n_cases, n_calls, 0, 0, 1);
        int32_t w[kG722Words];
        if (!g722_init_words(w, rate, options))
            fail("the configuration is refused", n_cases, 0, 0, rate, 0);
        // ---- the fixture's schedule: every call against the reference ----
        G722 s;
        g722_load(s, w, 1);
        std::vector<int32_t> got;
        int at = 0;
        for (int k = 0;  k < n_calls;  k++)
        {
            const size_t before = got.size();
            const int made = run_call(kind, s, data.data() + at, calls[k].len, got, n_cases, k);
            at += calls[k].len;
            if (made != calls[k].count)
                fail("count of call", n_cases, k, k, made, calls[k].count);
            for (size_t i = before;  i < got.size();  i++)
            {
                if (i >= want.size()  ||  got[i] != want[i])
                    fail("output", n_cases, k, (long long) i, got[i], (i < want.size())  ?  want[i]  :  -1);
            }
            g722_store(s, w, 1);
            for (int i = 0;  i < kG722Words;  i++)
            {
                if (w[i] != calls[k].words[i])
                    fail("state word", n_cases, k, i, w[i], calls[k].words[i]);
            }
            // (the next call starts from the words, as a launch does)
            g722_load(s, w, 1);
        }
        if (at != n_in  ||  got.size() != want.size())
            fail("items", n_cases, n_calls, at, (long long) got.size(), (long long) want.size());
        // ---- another cut of the same stream ----
        // (a call of a packed decoder ends with the code its last byte completed and whole codes may wait for the next call,
        // which starts with them: the loop goes through the same steps however the bytes are cut)
        static const int other[2][3] = {{4, 6, 160}, {3, 5, 160}};
        (void) g722_init_words(w, rate, options);
        g722_load(s, w, 1);
        std::vector<int32_t> again;
        at = 0;
        for (int k = 0;  at < n_in;  k++)
        {
            const int n = (other[kind][k % 3] < n_in - at)  ?  other[kind][k % 3]  :  (n_in - at);
            (void) run_call(kind, s, data.data() + at, n, again, n_cases, -k);
            at += n;
            g722_store(s, w, 1);
            g722_load(s, w, 1);
        }
        if (again != got)
            fail("the second schedule's output differs, items", n_cases, -1, 0, (long long) again.size(), (long long) got.size());
        for (int i = 0;  i < kG722Words;  i++)
        {
            if (w[i] != calls[n_calls - 1].words[i])
                fail("state word after the second schedule", n_cases, -1, i, w[i], calls[n_calls - 1].words[i]);
        }
        n_items += n_in;
        n_cases++;
    }
    fclose(in);
    if (slack[0] > 1  ||  slack[1] > 1)
    {
        fprintf(stderr, "no call came within one code of its capacity: encode %lld, decode %lld\n", slack[0], slack[1]);
        return 1;
    }
    printf("capacity slack: encode %lld, decode %lld\n", slack[0], slack[1]);
    printf("ok %d cases, %lld items\n", n_cases, n_items);
    return 0;
}
