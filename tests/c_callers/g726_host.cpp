// g726_host.cpp -- the per-sample functions of spandsp_amd/csrc/g726_dev.hpp compiled for the host and run one lane at a time
// over every case of tests/golden/g726.npz (tests/test_g726.py writes the cases out as whitespace separated integers and
// builds this file with -fsanitize=address,undefined).  Exit status 0 and "ok ..." on the last line: every code, packed
// byte, sample, count and state word equals the reference's under the fixture's call schedule; the same streams cut into
// calls of 3, 5, 160 give the same output and the same final state; and no call passed the capacity functions, which some
// call came within one unit of.
//
//   g726_host <cases file>
//
// The file: records that start with a letter.
//   C kind rate coding packing n_in n_out n_calls         kind 0: encode (in: row elements, out: bytes), 1: decode
//     n_in inputs, n_out outputs
//     n_calls x: len count check [30 words]                 check 1: the state words after the call follow
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/g726_dev.hpp"

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
    int len, count, check;
    int32_t words[kG726Words];
};

// one call of one channel, as a lane of the kernels makes it
static int encode_call(G726 &s, const int32_t *row, int n, std::vector<int32_t> &out)
{
    int made = 0;
    for (int i = 0;  i < n;  i++)
    {
        const int32_t code = g726_encode_sample(s, kG726TabHost, g726_linearize(s.coding, row[i]));
        int32_t byte;
        if (g726_pack(s, code, &byte))
        {
            out.push_back(byte);
            made++;
        }
    }
    return made;
}

static int decode_call(G726 &s, const int32_t *bytes, int n, std::vector<int32_t> &out)
{
    const int announced = g726_decode_count(s, n);
    int made = 0;
    for (int i = 0;  ;  )
    {
        int32_t byte = 0;
        if (g726_unpack_needs(s))
        {
            if (i >= n)
                break;
            byte = bytes[i++];
        }
        const int32_t code = g726_unpack(s, byte);
        int32_t v = g726_decode_code(s, kG726TabHost, code);
        // an element of the caller's row: an int16_t, or a G.711 byte
        out.push_back((s.coding == kG726Linear)  ?  v  :  (v & 0xFF));
        made++;
    }
    if (made != announced)
    {
        fprintf(stderr, "g726_decode_count() said %d, the loop made %d\n", announced, made);
        exit(1);
    }
    return made;
}

static long long slack[2] = {1 << 30, 1 << 30};

static int run_call(int kind, G726 &s, const int32_t *data, int n, std::vector<int32_t> &out, int case_no, int call)
{
    const int bps = s.bps;
    const int made = kind  ?  decode_call(s, data, n, out)  :  encode_call(s, data, n, out);
    const long long cap = kind  ?  g726_decode_capacity(bps, s.packing, n)  :  g726_encode_capacity(bps, s.packing, n);
    if (made > cap)
        fail("capacity passed, len", case_no, call, n, made, cap);
    if (cap - made < slack[kind])
        slack[kind] = cap - made;
    return made;
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: g726_host <cases file>\n");
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
        const int coding = next_int();
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
            c.check = next_int();
            if (c.check)
            {
                for (int w = 0;  w < kG726Words;  w++)
                    c.words[w] = next_int();
            }
        }
        if (n_calls == 0  ||  !calls[n_calls - 1].check)
            fail("no final state in the case", n_cases, n_calls, 0, 0, 1);
        int32_t w[kG726Words];
        if (!g726_init_words(w, rate, coding, packing))
            fail("g726_init refused", n_cases, 0, 0, rate, 0);
        // ---- the fixture's schedule: every call against the reference ----
        G726 s;
        g726_load(s, w, 1);
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
            g726_store(s, w, 1);
            if (calls[k].check)
            {
                for (int i = 0;  i < kG726Words;  i++)
                {
                    if (w[i] != calls[k].words[i])
                        fail("state word", n_cases, k, i, w[i], calls[k].words[i]);
                }
            }
        }
        if (at != n_in  ||  got.size() != want.size())
            fail("items", n_cases, n_calls, at, (long long) got.size(), (long long) want.size());
        // ---- another cut of the same stream: 3, 5, 160, cycled ----
        static const int other[3] = {3, 5, 160};
        (void) g726_init_words(w, rate, coding, packing);
        g726_load(s, w, 1);
        std::vector<int32_t> again;
        at = 0;
        for (int k = 0;  at < n_in;  k++)
        {
            const int n = (other[k % 3] < n_in - at)  ?  other[k % 3]  :  (n_in - at);
            (void) run_call(kind, s, data.data() + at, n, again, n_cases, -k);
            at += n;
        }
        g726_store(s, w, 1);
        if (again != got)
            fail("the second schedule's output differs, items", n_cases, -1, 0, (long long) again.size(), (long long) got.size());
        for (int i = 0;  i < kG726Words;  i++)
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
        fprintf(stderr, "no call came within one unit of its capacity: encode %lld, decode %lld\n", slack[0], slack[1]);
        return 1;
    }
    printf("capacity slack: encode %lld, decode %lld\n", slack[0], slack[1]);
    printf("ok %d cases, %lld items\n", n_cases, n_items);
    return 0;
}
