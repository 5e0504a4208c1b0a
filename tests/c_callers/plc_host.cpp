// plc_host.cpp -- the per-line functions of spandsp_amd/csrc/plc_dev.hpp compiled for the host and run one line at a time over
// every case of tests/golden/plc.npz (tests/test_plc.py writes the cases out as whitespace separated integers and builds this
// file with -fsanitize=address,undefined).  Exit status 0 and "ok ..." on the last line: every sample and every one of the 404
// state words equals the reference's after every call; the pitch search, through the kernel's per-lag sum and pair
// combination, finds the same lag in two orders of combination (upward, and the kernel's halving tree over 64 lanes after the
// fold of lags 104 .. 120); nothing is written to a row but what the header says; and the same streams with their heard
// stretches cut into calls of other lengths give the same samples and the same last 280 samples.
//
//   plc_host <cases file>
//
// The file: records that start with a letter.
//   C n_calls
//     n_calls x: lost len, len samples in, len samples out, 404 words: the state words after the call
//   E: the end

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/plc_dev.hpp"

using namespace spg;

static FILE *in;
static long searches;
static long most_tied;

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

static const int16_t kSentinel = 0x5A5A;

struct Call
{
    int lost, len;
    std::vector<int16_t> row, out;
    int32_t words[kPlcWords];
};

// a line's memory: its words, and a row with room for the chunk its last sample lies in and a chunk of sentinels behind it
struct HostMem
{
    int32_t *w;
    std::vector<int16_t> row;

    int32_t hist(int i) const { return w[PW_HISTORY + i]; }
    void set_hist(int i, int32_t v) { w[PW_HISTORY + i] = v; }
    float pb(int i) const
    {
        float f;
        memcpy(&f, &w[PW_PITCHBUF + i], sizeof(f));
        return f;
    }
    void set_pb(int i, float f) { memcpy(&w[PW_PITCHBUF + i], &f, sizeof(f)); }
    void set_row(int i, int32_t v) { row.at(i) = (int16_t) v; }
    void row_load8(int k, int16_t v[8]) const
    {
        for (int e = 0;  e < 8;  e++)
            v[e] = row.at(8*k + e);
    }
    void row_store8(int k, const int16_t v[8])
    {
        for (int e = 0;  e < 8;  e++)
            row.at(8*k + e) = v[e];
    }
};

// the search as the wave makes it (lane L: lag 40 + L, and 104 + L below lane 17; then the halving tree) against the search
// as the reference's loop makes it
static int search(const int16_t *amp)
{
    int32_t acc[64], lag[64];
    for (int lane = 0;  lane < 64;  lane++)
    {
        lag[lane] = kPlcLagFirst + lane;
        acc[lane] = plc_lag_sum(amp, lag[lane]);
        if (lane <= kPlcLagLast - kPlcLagFirst - 64)
            plc_pair_min(acc[lane], lag[lane], plc_lag_sum(amp, lag[lane] + 64), lag[lane] + 64);
    }
    for (int off = 32;  off > 0;  off >>= 1)
    {
        int32_t a2[64], l2[64];
        for (int lane = 0;  lane < 64;  lane++)
        {
            a2[lane] = acc[lane ^ off];
            l2[lane] = lag[lane ^ off];
        }
        for (int lane = 0;  lane < 64;  lane++)
            plc_pair_min(acc[lane], lag[lane], a2[lane], l2[lane]);
    }
    for (int lane = 1;  lane < 64;  lane++)
    {
        if (lag[lane] != lag[0]  ||  acc[lane] != acc[0])
            fail("the tree leaves the lanes apart at lane", -1, -1, lane, lag[lane], lag[0]);
    }
    // downward, so that a tie is met from the other side
    int32_t best = plc_lag_sum(amp, kPlcLagLast);
    int32_t best_lag = kPlcLagLast;
    long tied = 0;
    for (int l = kPlcLagLast - 1;  l >= kPlcLagFirst;  l--)
        plc_pair_min(best, best_lag, plc_lag_sum(amp, l), l);
    for (int l = kPlcLagFirst;  l <= kPlcLagLast;  l++)
        tied += (plc_lag_sum(amp, l) == best);
    if (best_lag != lag[0])
        fail("the two orders of combination disagree", -1, -1, 0, lag[0], best_lag);
    searches++;
    most_tied = (tied > most_tied)  ?  tied  :  most_tied;
    return best_lag;
}

// one call of one line, as a lane of the kernel makes it: from the words and back to them
static void one_call(int32_t *w, HostMem &m, int lost, int len)
{
    Plc s = {w[PW_MISSING], w[PW_OFFSET], w[PW_PITCH], w[PW_BUF_PTR]};
    if (lost  &&  s.missing == 0)
    {
        int16_t amp[kPlcHist];
        for (int i = 0;  i < kPlcHist;  i++)
            amp[i] = (int16_t) w[PW_HISTORY + plc_ring(s.buf_ptr + i)];
        s.pitch = search(amp);
        for (int i = 0;  i < kPlcHist;  i++)
            w[PW_HISTORY + i] = amp[i];
        s.buf_ptr = 0;
    }
    if (lost)
        plc_fillin_line(m, s, len);
    else
        plc_rx_line(m, s, len);
    w[PW_MISSING] = s.missing;
    w[PW_OFFSET] = s.offset;
    w[PW_PITCH] = s.pitch;
    w[PW_BUF_PTR] = s.buf_ptr;
}

static void give_row(HostMem &m, const int16_t *row, int len)
{
    m.row.assign((size_t) ((len + 7) & ~7) + 8, kSentinel);
    for (int i = 0;  i < len;  i++)
        m.row[i] = row[i];
}

static void check_row(const HostMem &m, const Call &c, int overlap_most, int case_no, int k)
{
    for (int i = 0;  i < c.len;  i++)
    {
        if (m.row[i] != c.out[i])
            fail("sample", case_no, k, i, m.row[i], c.out[i]);
    }
    const int edge = (c.len + 7) & ~7;
    for (int i = c.len;  i < (int) m.row.size();  i++)
    {
        // a filled row is zeros up to the chunk's end; everything else is as it was given
        const int want = (c.lost  &&  i < edge)  ?  0  :  kSentinel;
        if (m.row[i] != want)
            fail("past the length, sample", case_no, k, i, m.row[i], want);
    }
    if (!c.lost)
    {
        for (int i = overlap_most;  i < c.len;  i++)
        {
            if (m.row[i] != c.row[i])
                fail("a heard sample past the overlap changed:", case_no, k, i, m.row[i], c.row[i]);
        }
    }
}

static void run_case(const std::vector<Call> &calls, int case_no, long *n_calls)
{
    int32_t w[kPlcWords];
    int32_t w2[kPlcWords];
    memset(w, 0, sizeof(w));
    memset(w2, 0, sizeof(w2));
    for (size_t k = 0;  k < calls.size();  k++)
    {
        const Call &c = calls[k];
        if (!plc_words_ok(w))
            fail("words the bank would refuse before call", case_no, (int) k, 0, 0, 0);
        const int overlap_most = (!c.lost  &&  w[PW_MISSING])  ?  (w[PW_PITCH] >> 2)  :  0;
        HostMem m = {w, {}};
        give_row(m, c.row.data(), c.len);
        one_call(w, m, c.lost, c.len);
        check_row(m, c, overlap_most, case_no, (int) k);
        for (int i = 0;  i < kPlcWords;  i++)
        {
            if (w[i] != c.words[i])
                fail("state word", case_no, (int) k, i, w[i], c.words[i]);
        }
        // the second cut: a heard call with nothing missing before it, in pieces of 37
        HostMem m2 = {w2, {}};
        if (c.lost  ||  w2[PW_MISSING])
        {
            give_row(m2, c.row.data(), c.len);
            one_call(w2, m2, c.lost, c.len);
            check_row(m2, c, overlap_most, case_no, (int) k);
        }
        else
        {
            for (int at = 0;  at < c.len;  at += 37)
            {
                const int piece = (c.len - at > 37)  ?  37  :  (c.len - at);
                give_row(m2, c.row.data() + at, piece);
                one_call(w2, m2, 0, piece);
                for (int i = 0;  i < (int) m2.row.size();  i++)
                {
                    const int want = (i < piece)  ?  c.out[at + i]  :  kSentinel;
                    if (m2.row[i] != want)
                        fail("second cut, sample", case_no, (int) k, at + i, m2.row[i], want);
                }
            }
        }
        for (int i = 0;  i < PW_HISTORY;  i++)
        {
            if (w2[i] != w[i])
                fail("second cut, state word", case_no, (int) k, i, w2[i], w[i]);
        }
        for (int i = 0;  i < kPlcHist;  i++)
        {
            const int32_t a = w[PW_HISTORY + plc_ring(w[PW_BUF_PTR] % kPlcHist + i)];
            const int32_t b = w2[PW_HISTORY + plc_ring(w2[PW_BUF_PTR] % kPlcHist + i)];
            if (a != b)
                fail("second cut, history in time order at", case_no, (int) k, i, b, a);
        }
        (*n_calls)++;
    }
}

int main(int argc, char **argv)
{
    if (argc != 2  ||  (in = fopen(argv[1], "r")) == NULL)
    {
        fprintf(stderr, "usage: plc_host <cases file>\n");
        return 2;
    }
    int n_cases = 0;
    long n_calls = 0;
    char tag[4];
    while (fscanf(in, "%1s", tag) == 1  &&  tag[0] == 'C')
    {
        std::vector<Call> calls((size_t) next_int());
        for (Call &c : calls)
        {
            c.lost = next_int();
            c.len = next_int();
            c.row.resize((size_t) c.len);
            c.out.resize((size_t) c.len);
            for (int i = 0;  i < c.len;  i++)
                c.row[i] = (int16_t) next_int();
            for (int i = 0;  i < c.len;  i++)
                c.out[i] = (int16_t) next_int();
            for (int i = 0;  i < kPlcWords;  i++)
                c.words[i] = next_int();
        }
        run_case(calls, n_cases, &n_calls);
        n_cases++;
    }
    fclose(in);
    if (tag[0] != 'E')
    {
        fprintf(stderr, "cases file: no end record\n");
        return 2;
    }
    printf("searches: %ld, the most lags tied %ld\n", searches, most_tied);
    printf("ok %d cases, %ld calls\n", n_cases, n_calls);
    return 0;
}
