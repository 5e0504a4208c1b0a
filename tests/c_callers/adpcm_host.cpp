// adpcm_host.cpp -- the per-item functions and per-call bodies of csrc/adpcm_dev.hpp compiled for the host, one lane at a time:
// a stand-alone program (tests/test_adpcm.py builds it with -fsanitize=address,undefined) that reads cases as
// tests/adpcm_lines.py dump_text() writes them and checks, call by call, outputs, counts and state words; that a second cut of
// every stream that may be cut gives the same stream; that no call reads outside what it was given or makes more than its
// capacity function says; and the three documented deviations from the reference.
//
//   adpcm_host <cases.txt>
//   adpcm_host --run <cases.txt>    checks nothing: prints what every case makes ("O" and its items, then per call "K", the
//                                   count and the state words), for a test that holds a bank against these functions
//
// It ends with "ok <n> cases" and "capacity slack: ..." (the least distance, over all calls, between a count and its
// capacity), or with the first difference and status 1.

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/adpcm_dev.hpp"

using namespace spg;

enum { IMA = 0, OKI = 1, ENCODE = 0, DECODE = 1 };

static void fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    printf("FAILED: %s (%ld %ld %ld)\n", what, a, b, c);
    exit(1);
}

// a call's input: reading past it ends the program
struct HostIn
{
    const int32_t *v;
    int n;
    int at;

    int32_t next()
    {
        if (at >= n)
            fail("a call read past its input", at, n);
        return v[at++];
    }
    int32_t u8() { return next() & 0xFF; }
    int32_t s16() { return adpcm_s16(next()); }
};

// a call's output: passing the capacity ends the program
struct HostOut
{
    std::vector<int32_t> *v;
    size_t start;
    long cap;

    void put(int32_t x)
    {
        if ((long) (v->size() - start) >= cap)
            fail("a call passed its capacity", cap);
        v->push_back(x);
    }
    void put8(int32_t x) { put(x & 0xFF); }
    void put16(int32_t x) { put(adpcm_s16(x)); }
};

struct HostHist
{
    int32_t *w;

    int32_t get(int i) const { return w[i]; }
    void set(int i, int32_t x) { w[i] = x; }
};

struct Lane
{
    int family;
    int32_t w[kOkiWords];
};

static int words_of(int family)
{
    return (family == IMA)  ?  (int) kImaWords  :  (int) kOkiWords;
}

static void lane_init(Lane &l, int family, int a, int b, int entry_phase)
{
    l.family = family;
    memset(l.w, 0, sizeof(l.w));
    if (!((family == IMA)  ?  ima_init_words(l.w, a, b)  :  oki_init_words(l.w, a)))
        fail("init refused a configuration", family, a, b);
    if (family == OKI)
        l.w[OK_PHASE] = entry_phase;
}

static long capacity(const Lane &l, int kind, int len)
{
    if (l.family == IMA)
        return (kind == ENCODE)  ?  ima_encode_capacity(l.w[IM_VARIANT], l.w[IM_CHUNK] == 0, len)  :  ima_decode_capacity(l.w[IM_VARIANT], l.w[IM_CHUNK] == 0, len);
    return (kind == ENCODE)  ?  oki_encode_capacity(l.w[OK_RATE], len)  :  oki_decode_capacity(l.w[OK_RATE], len);
}

// one call of one lane, as a kernel's lane makes it; returns the count
static int lane_call(Lane &l, int kind, const int32_t *data, int len, std::vector<int32_t> &out)
{
    HostIn in = {data, len, 0};
    HostOut o = {&out, out.size(), capacity(l, kind, len)};
    if (l.family == IMA)
    {
        Ima s = {l.w[IM_VARIANT], l.w[IM_CHUNK], l.w[IM_LAST], l.w[IM_STEP], l.w[IM_BYTE], l.w[IM_BITS]};
        if (kind == ENCODE)
            ima_encode_call(s, kAdpcmStepHost, in, o, len);
        else
            ima_decode_call(s, kAdpcmStepHost, in, o, len);
        l.w[IM_LAST] = s.last;
        l.w[IM_STEP] = s.step;
        l.w[IM_BYTE] = s.byte;
        l.w[IM_BITS] = s.bits;
    }
    else
    {
        Oki s = {l.w[OK_RATE], l.w[OK_LAST], l.w[OK_STEP], l.w[OK_BYTE], l.w[OK_PTR], l.w[OK_MARK], l.w[OK_PHASE]};
        HostHist h = {l.w + OK_HIST};
        if (kind == ENCODE)
            oki_encode_call(s, kAdpcmStepHost, kAdpcmHalfHost, h, in, o, len);
        else
            oki_decode_call(s, kAdpcmStepHost, kAdpcmHalfHost, h, in, o, len);
        l.w[OK_LAST] = s.last;
        l.w[OK_STEP] = s.step;
        l.w[OK_BYTE] = s.byte;
        l.w[OK_PTR] = s.ptr;
        l.w[OK_MARK] = s.mark;
        l.w[OK_PHASE] = s.phase;
    }
    return (int) (out.size() - o.start);
}

static long slack[2][2] = {{1 << 30, 1 << 30}, {1 << 30, 1 << 30}};

static std::vector<int32_t> read_ints(FILE *f, int n)
{
    std::vector<int32_t> v((size_t) n);
    for (int i = 0;  i < n;  i++)
    {
        long x;
        if (fscanf(f, "%ld", &x) != 1)
            fail("short file");
        v[(size_t) i] = (int32_t) x;
    }
    return v;
}

static void deviations()
{
    static const int cfg[8][3] = {{IMA, 0, 0}, {IMA, 0, 64}, {IMA, 1, 0}, {IMA, 1, 64}, {IMA, 2, 0}, {IMA, 2, 64}, {OKI, 32000, 0}, {OKI, 24000, 0}};
    std::vector<int32_t> out;
    for (int i = 0;  i < 8;  i++)
    {
        for (int kind = ENCODE;  kind <= DECODE;  kind++)
        {
            // a length of 0 changes nothing, reads nothing and counts 0 -- from a state in mid stream
            Lane l;
            lane_init(l, cfg[i][0], cfg[i][1], cfg[i][2], 3);
            static const int32_t some[7] = {1000, -2000, 30000, -30000, 5, 0x7F, 0x80};
            (void) lane_call(l, kind, some, (kind == DECODE  &&  l.family == IMA  &&  cfg[i][2] == 0)  ?  7  :  5, out);
            Lane before = l;
            out.clear();
            if (lane_call(l, kind, NULL, 0, out) != 0  ||  memcmp(&before, &l, sizeof(l)) != 0)
                fail("a call of length 0 did something", i, kind);
            if (capacity(l, kind, 0) != 0)
                fail("capacity of nothing", i, kind);
        }
    }
    for (int variant = 0;  variant < 3;  variant++)
    {
        // a decode call with chunk_size == 0 and fewer than 4 bytes: nothing out, nothing read, the state alone
        for (int n = 1;  n < 4;  n++)
        {
            Lane l;
            lane_init(l, IMA, variant, 0, 0);
            l.w[IM_LAST] = -1234;
            l.w[IM_STEP] = 40;
            l.w[IM_BITS] = 5;
            Lane before = l;
            out.clear();
            if (lane_call(l, DECODE, NULL, n, out) != 0  ||  memcmp(&before, &l, sizeof(l)) != 0)
                fail("a short header call did something", variant, n);
        }
        // a header's step_index above 88 is 88
        static const int32_t high[8] = {0x12, 0x34, 200, 0, 0x7F, 0x80, 0x3C, 0xF1};
        static const int32_t top[8] = {0x12, 0x34, 88, 0, 0x7F, 0x80, 0x3C, 0xF1};
        Lane a, b;
        std::vector<int32_t> oa, ob;
        lane_init(a, IMA, variant, 0, 0);
        lane_init(b, IMA, variant, 0, 0);
        const int na = lane_call(a, DECODE, high, 8, oa);
        const int nb = lane_call(b, DECODE, top, 8, ob);
        if (na != nb  ||  na < 8  ||  oa != ob  ||  memcmp(&a, &b, sizeof(a)) != 0)
            fail("a header step_index above 88 is not taken as 88", variant, na, nb);
    }
}

int main(int argc, char **argv)
{
    const bool only_run = (argc == 3  &&  strcmp(argv[1], "--run") == 0);
    if (argc != 2  &&  !only_run)
        fail("usage: adpcm_host [--run] <cases.txt>");
    FILE *f = fopen(argv[argc - 1], "r");
    if (f == NULL)
        fail("cannot open the cases");
    int cases = 0;
    for (;;)
    {
        char tag[8];
        if (fscanf(f, "%7s", tag) != 1)
            fail("no end mark");
        if (tag[0] == 'E')
            break;
        int family, kind, a, b, recut, entry, ndata, nwant, ncalls;
        if (fscanf(f, "%d %d %d %d %d %d %d %d %d", &family, &kind, &a, &b, &recut, &entry, &ndata, &nwant, &ncalls) != 9)
            fail("bad case header", cases);
        const std::vector<int32_t> data = read_ints(f, ndata);
        const std::vector<int32_t> want = read_ints(f, nwant);
        const int nw = words_of(family);
        Lane l;
        lane_init(l, family, a, b, entry);
        std::vector<int32_t> out;
        std::vector<int32_t> last_words;
        int at = 0;
        if (only_run)
        {
            std::vector<int32_t> counts;
            std::vector<int32_t> after;
            for (int c = 0;  c < ncalls;  c++)
            {
                const int len = read_ints(f, 2 + nw)[0];
                if (at + len > ndata)
                    fail("calls longer than the data", cases, c);
                counts.push_back(lane_call(l, kind, data.data() + at, len, out));
                at += len;
                after.insert(after.end(), l.w, l.w + nw);
            }
            printf("O %zu", out.size());
            for (size_t i = 0;  i < out.size();  i++)
                printf(" %d", (int) out[i]);
            printf("\n");
            for (int c = 0;  c < ncalls;  c++)
            {
                printf("K %d", (int) counts[(size_t) c]);
                for (int i = 0;  i < nw;  i++)
                    printf(" %d", (int) after[(size_t) (c*nw + i)]);
                printf("\n");
            }
            cases++;
            continue;
        }
        for (int c = 0;  c < ncalls;  c++)
        {
            const std::vector<int32_t> head = read_ints(f, 2);
            const std::vector<int32_t> words = read_ints(f, nw);
            const int len = head[0];
            if (at + len > ndata)
                fail("calls longer than the data", cases, c);
            const size_t had = out.size();
            const int count = lane_call(l, kind, data.data() + at, len, out);
            at += len;
            if (count != head[1])
                fail("count", cases, c, count);
            for (size_t i = had;  i < out.size();  i++)
            {
                if (i >= want.size()  ||  out[i] != want[i])
                    fail("output", cases, c, (long) i);
            }
            for (int i = 0;  i < nw;  i++)
            {
                if (l.w[i] != words[(size_t) i])
                    fail("state word", cases, c, i);
            }
            const long s = capacity(l, kind, len) - count;
            slack[family][kind] = (s < slack[family][kind])  ?  s  :  slack[family][kind];
            last_words = words;
        }
        if (out.size() != want.size()  ||  at != ndata)
            fail("stream length", cases, (long) out.size(), (long) want.size());
        if (recut)
        {
            // the same stream cut another way: the same items and the same last words
            static const int other[5] = {5, 64, 1, 9, 2};
            Lane m;
            lane_init(m, family, a, b, entry);
            std::vector<int32_t> again;
            int k = 0;
            for (at = 0;  at < ndata;  k++)
            {
                const int len = (ndata - at < other[k % 5])  ?  (ndata - at)  :  other[k % 5];
                (void) lane_call(m, kind, data.data() + at, len, again);
                at += len;
            }
            if (again != want)
                fail("a second cut gives another stream", cases);
            for (int i = 0;  i < nw  &&  ncalls > 0;  i++)
            {
                if (m.w[i] != last_words[(size_t) i])
                    fail("a second cut ends on other words", cases, i);
            }
        }
        cases++;
    }
    fclose(f);
    if (only_run)
        return 0;
    deviations();
    printf("ok %d cases\n", cases);
    printf("capacity slack: ima encode %ld, ima decode %ld, oki encode %ld, oki decode %ld\n", slack[IMA][ENCODE], slack[IMA][DECODE], slack[OKI][ENCODE],
           slack[OKI][DECODE]);
    return 0;
}
