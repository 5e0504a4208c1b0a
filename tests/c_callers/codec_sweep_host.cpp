// codec_sweep_host.cpp -- the per-sample, per-frame and per-line functions of spandsp_amd/csrc/g726_dev.hpp, g722_dev.hpp,
// gsm0610_dev.hpp and plc_dev.hpp compiled for the host and run one lane at a time over the generated lines of the codec sweep
// (tests/codec_sweep.py), beside the reference's own functions called on the same input: tests/test_codec_sweep.py writes the
// lines, configurations and schedules to binary files, builds this file with -fsanitize=address,undefined and links it against
// oracle/_ref/libspandsp_codecs_ref.so.  Every output item, every count and every state word must be equal after every call.
// Exit status 0 and "ok ..." on the last line, or the first difference as family, line, call and index.
//
//   codec_sweep_host <file> ...
//
// A file: int32 words, little-endian.
//   0x53574550, records
//   a record: family (0 G.726, 1 G.722, 2 GSM 06.10, 3 concealer), kind (0 encode, 1 decode), three configuration words, line,
//             n_calls, n_bytes, n_calls lengths, n_calls lost flags, then n_bytes bytes of input items padded to a whole word
//             (int16 samples or bytes, as the reference's function takes them; of the concealer the rows one behind the other)
//
// The concealer's pitch search goes through the kernel's per-lag sum, the fold of lags 104 .. 120 and the halving tree.

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spandsp_amd/csrc/g726_dev.hpp"
#include "../../spandsp_amd/csrc/g722_dev.hpp"
#include "../../spandsp_amd/csrc/gsm0610_dev.hpp"
#include "../../spandsp_amd/csrc/plc_dev.hpp"

using namespace spg;

// the reference, as its public headers declare it, and the state accessors of oracle/ref_glue/ref_glue_codecs.c
extern "C"
{
void *g726_init(void *s, int bit_rate, int ext_coding, int packing);
int g726_free(void *s);
int g726_encode(void *s, uint8_t g726_data[], const int16_t amp[], int len);
int g726_decode(void *s, int16_t amp[], const uint8_t g726_data[], int g726_bytes);
void *g722_encode_init(void *s, int rate, int options);
int g722_encode_free(void *s);
int g722_encode(void *s, uint8_t g722_data[], const int16_t amp[], int len);
void *g722_decode_init(void *s, int rate, int options);
int g722_decode_free(void *s);
int g722_decode(void *s, int16_t amp[], const uint8_t g722_data[], int len);
void *gsm0610_init(void *s, int packing);
int gsm0610_free(void *s);
int gsm0610_encode(void *s, uint8_t code[], const int16_t amp[], int len);
int gsm0610_decode(void *s, int16_t amp[], const uint8_t code[], int len);
void *plc_init(void *s);
int plc_free(void *s);
int plc_rx(void *s, int16_t amp[], int len);
int plc_fillin(void *s, int16_t amp[], int len);
int glue_g726_words(const void *s, int32_t w[]);
int glue_g722_words(int kind, const void *s, int32_t w[]);
int glue_gsm0610_words(const void *s, int32_t w[]);
int glue_plc_words(const void *s, int32_t w[]);
}

static const char *const kFamily[4] = {"g726", "g722", "gsm0610", "plc"};

struct Record
{
    int family, kind, cfg[3], line, n_calls;
    std::vector<int32_t> lens, lost;
    std::vector<uint8_t> data;
};

static void fail(const Record &r, int call, const char *what, long long at, long long got, long long want)
{
    fprintf(stderr, "%s %s, configuration (%d, %d, %d), line %d, call %d: %s %lld: got %lld, the reference has %lld\n", kFamily[r.family],
            (r.family == 3)  ?  ""  :  (r.kind  ?  "decode"  :  "encode"), r.cfg[0], r.cfg[1], r.cfg[2], r.line, call, what, at, got, want);
    exit(1);
}

static void same_words(const Record &r, int call, const int32_t *mine, const int32_t *ref, int n)
{
    for (int i = 0;  i < n;  i++)
    {
        if (mine[i] != ref[i])
            fail(r, call, "state word", i, mine[i], ref[i]);
    }
}

static void same_items(const Record &r, int call, const std::vector<int32_t> &mine, const std::vector<int32_t> &ref)
{
    if (mine.size() != ref.size())
        fail(r, call, "count, call", call, (long long) mine.size(), (long long) ref.size());
    for (size_t i = 0;  i < mine.size();  i++)
    {
        if (mine[i] != ref[i])
            fail(r, call, "output item", (long long) i, mine[i], ref[i]);
    }
}

static long long n_items[4], n_calls_made[4], n_lines[4];

// ---- G.726 ----------------------------------------------------------------------------------------------------------------

static void run_g726(const Record &r)
{
    const int rate = r.cfg[0], coding = r.cfg[1], packing = r.cfg[2];
    const int el = (r.kind == 0  &&  coding == kG726Linear)  ?  2  :  1;
    void *ref = g726_init(NULL, rate, coding, packing);
    int32_t w[kG726Words], wr[kG726Words];
    if (ref == NULL  ||  !g726_init_words(w, rate, coding, packing))
        fail(r, -1, "init refused, rate", 0, rate, 0);
    G726 s;
    size_t at = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        const int n = r.lens[k];
        if (n == 0)
            continue;
        std::vector<int32_t> in(n), mine, theirs;
        // (copies of exactly the call's size, so that the sanitizer sees a read past either)
        std::vector<uint8_t> raw(r.data.begin() + at, r.data.begin() + at + (size_t) n*el);
        at += (size_t) n*el;
        for (int i = 0;  i < n;  i++)
            in[i] = (el == 2)  ?  (int32_t) (int16_t) (raw[2*i] | (raw[2*i + 1] << 8))  :  raw[i];
        g726_load(s, w, 1);
        if (r.kind == 0)
        {
            std::vector<uint8_t> out(n + 1);
            const int made = g726_encode(ref, out.data(), (const int16_t *) (const void *) raw.data(), n);
            theirs.assign(out.begin(), out.begin() + made);
            for (int i = 0;  i < n;  i++)
            {
                const int32_t code = g726_encode_sample(s, kG726TabHost, g726_linearize(s.coding, in[i]));
                int32_t byte;
                if (g726_pack(s, code, &byte))
                    mine.push_back(byte);
            }
            if ((long long) mine.size() > g726_encode_capacity(s.bps, s.packing, n))
                fail(r, k, "capacity passed, len", n, (long long) mine.size(), g726_encode_capacity(s.bps, s.packing, n));
        }
        else
        {
            std::vector<int16_t> out(4*n + 8);
            const int made = g726_decode(ref, out.data(), raw.data(), n);
            for (int i = 0;  i < made;  i++)
                theirs.push_back((coding == kG726Linear)  ?  (int32_t) out[i]  :  (int32_t) ((const uint8_t *) (const void *) out.data())[i]);
            const int announced = g726_decode_count(s, n);
            for (int i = 0;  ;  )
            {
                int32_t byte = 0;
                if (g726_unpack_needs(s))
                {
                    if (i >= n)
                        break;
                    byte = in[i++];
                }
                const int32_t v = g726_decode_code(s, kG726TabHost, g726_unpack(s, byte));
                mine.push_back((s.coding == kG726Linear)  ?  v  :  (v & 0xFF));
            }
            if ((int) mine.size() != announced)
                fail(r, k, "g726_decode_count(), len", n, announced, (long long) mine.size());
            if ((long long) mine.size() > g726_decode_capacity(s.bps, s.packing, n))
                fail(r, k, "capacity passed, len", n, (long long) mine.size(), g726_decode_capacity(s.bps, s.packing, n));
        }
        g726_store(s, w, 1);
        same_items(r, k, mine, theirs);
        glue_g726_words(ref, wr);
        same_words(r, k, w, wr, kG726Words);
        n_items[0] += n;
        n_calls_made[0]++;
    }
    g726_free(ref);
}

// ---- G.722 ----------------------------------------------------------------------------------------------------------------

static void run_g722(const Record &r)
{
    const int rate = r.cfg[0], options = r.cfg[1];
    const int el = (r.kind == 0)  ?  2  :  1;
    void *ref = (r.kind == 0)  ?  g722_encode_init(NULL, rate, options)  :  g722_decode_init(NULL, rate, options);
    int32_t w[kG722Words], wr[kG722Words];
    if (ref == NULL  ||  !g722_init_words(w, rate, options))
        fail(r, -1, "init refused, rate", 0, rate, 0);
    G722 s;
    size_t at = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        const int n = r.lens[k];
        if (n == 0)
            continue;
        std::vector<int32_t> mine, theirs;
        std::vector<uint8_t> raw(r.data.begin() + at, r.data.begin() + at + (size_t) n*el);
        at += (size_t) n*el;
        g722_load(s, w, 1);
        if (r.kind == 0)
        {
            std::vector<int16_t> amp(n);
            memcpy(amp.data(), raw.data(), raw.size());
            std::vector<uint8_t> out(n + 8);
            const int made = g722_encode(ref, out.data(), amp.data(), n);
            theirs.assign(out.begin(), out.begin() + made);
            const int per = s.eight_k  ?  1  :  2;
            for (int i = 0;  i + per <= n;  i += per)
            {
                const int32_t code = g722_encode_code(s, kG722TabHost, amp[i] & 0xFFFF, (per == 2)  ?  (amp[i + 1] & 0xFFFF)  :  0);
                int32_t byte;
                if (g722_pack(s, code, &byte))
                    mine.push_back(byte);
            }
            if ((long long) mine.size() > g722_encode_capacity(s.bps, s.packed, s.eight_k, n))
                fail(r, k, "capacity passed, len", n, (long long) mine.size(), g722_encode_capacity(s.bps, s.packed, s.eight_k, n));
        }
        else
        {
            std::vector<int16_t> out(3*n + 16);
            const int made = g722_decode(ref, out.data(), raw.data(), n);
            theirs.assign(out.begin(), out.begin() + made);
            const int announced = g722_decode_codes(s, n);
            int codes = 0;
            for (int i = 0;  i < n;  codes++)
            {
                int32_t byte = 0;
                if (g722_unpack_needs(s))
                    byte = raw[i++];
                int32_t amp[2];
                g722_decode_code(s, kG722TabHost, g722_unpack(s, byte), amp);
                mine.push_back(amp[0]);
                if (!s.eight_k)
                    mine.push_back(amp[1]);
            }
            if (codes != announced)
                fail(r, k, "g722_decode_codes(), len", n, announced, codes);
            if ((long long) mine.size() > g722_decode_capacity(s.bps, s.packed, s.eight_k, n))
                fail(r, k, "capacity passed, len", n, (long long) mine.size(), g722_decode_capacity(s.bps, s.packed, s.eight_k, n));
        }
        g722_store(s, w, 1);
        same_items(r, k, mine, theirs);
        glue_g722_words(r.kind, ref, wr);
        same_words(r, k, w, wr, kG722Words);
        n_items[1] += n;
        n_calls_made[1]++;
    }
    if (r.kind == 0)
        g722_encode_free(ref);
    else
        g722_decode_free(ref);
}

// ---- GSM 06.10 ------------------------------------------------------------------------------------------------------------

struct ByteSink
{
    std::vector<int32_t> *out;
    void word(uint32_t w)
    {
        for (int i = 0;  i < 4;  i++)
            out->push_back((int32_t) ((w >> (8*i)) & 0xFF));
    }
};

static void run_gsm0610(const Record &r)
{
    const int packing = r.cfg[0];
    const int el = (r.kind == 0)  ?  2  :  1;
    void *ref = gsm0610_init(NULL, packing);
    int32_t w[kGsmWords], wr[kGsmWords];
    if (ref == NULL  ||  !gsm0610_init_words(w, packing))
        fail(r, -1, "init refused, packing", 0, packing, 0);
    size_t at = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        const int n = r.lens[k];
        if (n == 0)
            continue;
        std::vector<int32_t> mine, theirs;
        std::vector<uint8_t> raw(r.data.begin() + at, r.data.begin() + at + (size_t) n*el);
        at += (size_t) n*el;
        Gsm s;
        GsmHostMem m;
        memset(&m, 0, sizeof(m));
        gsm_load(s, w, 1);
        gsm_load_hist(m, w, 1);
        if (r.kind == 0)
        {
            std::vector<int16_t> amp(n);
            memcpy(amp.data(), raw.data(), raw.size());
            std::vector<uint8_t> out(n);
            const int made = gsm0610_encode(ref, out.data(), amp.data(), n);
            theirs.assign(out.begin(), out.begin() + made);
            ByteSink sink = {&mine};
            GsmBitsOut bits;
            gsm_bits_begin(bits, s.packing);
            for (int f = 0;  f < n/kGsmFrame;  f++)
            {
                for (int i = 0;  i < kGsmFrame;  i++)
                    m.st(kGsmHist + i, gsm_preprocess(s, amp[f*kGsmFrame + i] & 0xFFFF));
                gsm_encode_frame(s, m, bits, sink);
            }
            gsm_bits_end(bits, sink);
            // (the last word carries zeros past the count, as the last chunk of a row does)
            const size_t count = (size_t) gsm0610_encode_capacity(s.packing, n);
            if (mine.size() < count)
                fail(r, k, "the stream is shorter than the count, len", n, (long long) mine.size(), (long long) count);
            for (size_t i = count;  i < mine.size();  i++)
            {
                if (mine[i] != 0)
                    fail(r, k, "bits past the count, byte", (long long) i, mine[i], 0);
            }
            mine.resize(count);
        }
        else
        {
            std::vector<int16_t> out(5*n + 8);
            const int made = gsm0610_decode(ref, out.data(), raw.data(), n);
            theirs.assign(out.begin(), out.begin() + made);
            const int frames = (int) (gsm0610_decode_capacity(s.packing, n)/kGsmFrame);
            for (int f = 0;  f < frames;  f++)
            {
                const int start = (s.packing == kGsmWav49)  ?  ((f >> 1)*520 + (f & 1)*260)  :  (f*8*gsm0610_unit_bytes(s.packing));
                const int byte0 = start >> 3;
                // the stage starts at the 32-bit word of the row that holds the frame's first byte, as in the kernel
                const int from = byte0 & ~3;
                for (int i = 0;  i < kGsmStageBytes;  i++)
                    m.stage_byte(i, (uint8_t) ((from + i < n)  ?  raw[from + i]  :  0xFF));
                int32_t LARc[8], cur[8], prev[8], rrp[8];
                gsm_decode_residual(s, m, 8*(byte0 & 3) + (start & 7), LARc);
                gsm_decode_lar(s, LARc, cur, prev);
                for (int range = 0;  range < 4;  range++)
                {
                    gsm_range_rp(range, cur, prev, rrp);
                    for (int i = gsm_range_start(range);  i < gsm_range_start(range + 1);  i++)
                        mine.push_back(gsm_decode_sample(s, m, i, rrp));
                }
                gsm_shift_hist(m);
            }
        }
        gsm_store(s, w, 1);
        gsm_store_hist(m, w, 1);
        same_items(r, k, mine, theirs);
        glue_gsm0610_words(ref, wr);
        same_words(r, k, w, wr, kGsmWords);
        n_items[2] += n;
        n_calls_made[2]++;
    }
    gsm0610_free(ref);
}

// ---- the concealer --------------------------------------------------------------------------------------------------------

static const int16_t kSentinel = 0x5A5A;
static long long searches, tied_searches;

// a line's memory: its words, and a row with room for the chunk its last sample lies in and a chunk of sentinels behind it
struct PlcHostMem
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

// the search as the wave makes it: lane L takes lag 40 + L, and 104 + L below lane 17; then the halving tree
static int plc_search(const Record &r, int call, const int16_t *amp)
{
    int32_t acc[64], lag[64], sums[kPlcLagLast - kPlcLagFirst + 1];
    for (int l = kPlcLagFirst;  l <= kPlcLagLast;  l++)
        sums[l - kPlcLagFirst] = plc_lag_sum(amp, l);
    for (int lane = 0;  lane < 64;  lane++)
    {
        lag[lane] = kPlcLagFirst + lane;
        acc[lane] = sums[lane];
        if (lane <= kPlcLagLast - kPlcLagFirst - 64)
            plc_pair_min(acc[lane], lag[lane], sums[lane + 64], lag[lane] + 64);
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
            fail(r, call, "the tree leaves the lanes apart at lane", lane, lag[lane], lag[0]);
    }
    int tied = 0;
    for (int l = kPlcLagFirst;  l <= kPlcLagLast;  l++)
        tied += (sums[l - kPlcLagFirst] == acc[0]);
    searches++;
    tied_searches += (tied > 1);
    return lag[0];
}

static void run_plc(const Record &r)
{
    void *ref = plc_init(NULL);
    int32_t w[kPlcWords], wr[kPlcWords];
    memset(w, 0, sizeof(w));
    if (ref == NULL)
        fail(r, -1, "plc_init", 0, 0, 1);
    size_t at = 0;
    for (int k = 0;  k < r.n_calls;  k++)
    {
        const int n = r.lens[k];
        if (n == 0)
            continue;
        const int lost = r.lost[k];
        std::vector<int16_t> theirs(n);
        memcpy(theirs.data(), r.data.data() + at, 2*(size_t) n);
        at += 2*(size_t) n;
        if (!plc_words_ok(w))
            fail(r, k, "words the bank would refuse before the call", 0, 0, 0);
        PlcHostMem m = {w, {}};
        m.row.assign((size_t) ((n + 7) & ~7) + 8, kSentinel);
        memcpy(m.row.data(), theirs.data(), 2*(size_t) n);
        if (lost)
            plc_fillin(ref, theirs.data(), n);
        else
            plc_rx(ref, theirs.data(), n);
        // one call of one line, as a lane of the kernel makes it: from the words and back to them
        Plc s = {w[PW_MISSING], w[PW_OFFSET], w[PW_PITCH], w[PW_BUF_PTR]};
        if (lost  &&  s.missing == 0)
        {
            int16_t amp[kPlcHist];
            for (int i = 0;  i < kPlcHist;  i++)
                amp[i] = (int16_t) w[PW_HISTORY + plc_ring(s.buf_ptr + i)];
            s.pitch = plc_search(r, k, amp);
            for (int i = 0;  i < kPlcHist;  i++)
                w[PW_HISTORY + i] = amp[i];
            s.buf_ptr = 0;
        }
        if (lost)
            plc_fillin_line(m, s, n);
        else
            plc_rx_line(m, s, n);
        w[PW_MISSING] = s.missing;
        w[PW_OFFSET] = s.offset;
        w[PW_PITCH] = s.pitch;
        w[PW_BUF_PTR] = s.buf_ptr;
        for (int i = 0;  i < n;  i++)
        {
            if (m.row[i] != theirs[i])
                fail(r, k, "sample", i, m.row[i], theirs[i]);
        }
        // a filled row is zeros up to the chunk's end; everything else is as it was given
        const int edge = (n + 7) & ~7;
        for (int i = n;  i < (int) m.row.size();  i++)
        {
            const int want = (lost  &&  i < edge)  ?  0  :  kSentinel;
            if (m.row[i] != want)
                fail(r, k, "past the length, sample", i, m.row[i], want);
        }
        glue_plc_words(ref, wr);
        same_words(r, k, w, wr, kPlcWords);
        n_items[3] += n;
        n_calls_made[3]++;
    }
    plc_free(ref);
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
    if (in == NULL  ||  next_word(in, path) != 0x53574550)
    {
        fprintf(stderr, "%s: not a sweep file\n", path);
        exit(2);
    }
    const int records = next_word(in, path);
    for (int i = 0;  i < records;  i++)
    {
        Record r;
        r.family = next_word(in, path);
        r.kind = next_word(in, path);
        for (int c = 0;  c < 3;  c++)
            r.cfg[c] = next_word(in, path);
        r.line = next_word(in, path);
        r.n_calls = next_word(in, path);
        const int n_bytes = next_word(in, path);
        if (r.family < 0  ||  r.family > 3  ||  r.n_calls < 0  ||  r.n_calls > 4096  ||  n_bytes < 0  ||  n_bytes > (1 << 24))
        {
            fprintf(stderr, "%s: record %d is no record\n", path, i);
            exit(2);
        }
        r.lens.resize((size_t) r.n_calls);
        r.lost.resize((size_t) r.n_calls);
        for (int32_t &v : r.lens)
            v = next_word(in, path);
        for (int32_t &v : r.lost)
            v = next_word(in, path);
        r.data.resize((size_t) (n_bytes + 3) & ~(size_t) 3);
        if (!r.data.empty()  &&  fread(r.data.data(), 1, r.data.size(), in) != r.data.size())
        {
            fprintf(stderr, "%s: cut short\n", path);
            exit(2);
        }
        r.data.resize((size_t) n_bytes);
        long long need = 0;
        for (int k = 0;  k < r.n_calls;  k++)
            need += r.lens[k];
        const int el = (r.family == 3  ||  (r.kind == 0  &&  !(r.family == 0  &&  r.cfg[1] != kG726Linear)))  ?  2  :  1;
        if (need*el != n_bytes)
        {
            fprintf(stderr, "%s: record %d: %lld items of %d bytes, %d bytes\n", path, i, need, el, n_bytes);
            exit(2);
        }
        switch (r.family)
        {
        case 0:
            run_g726(r);
            break;
        case 1:
            run_g722(r);
            break;
        case 2:
            run_gsm0610(r);
            break;
        default:
            run_plc(r);
            break;
        }
        n_lines[r.family]++;
    }
    fclose(in);
}

int main(int argc, char **argv)
{
    if (argc < 2)
    {
        fprintf(stderr, "usage: codec_sweep_host <file> ...\n");
        return 2;
    }
    for (int i = 1;  i < argc;  i++)
        run_file(argv[i]);
    for (int f = 0;  f < 4;  f++)
        printf("%s: %lld lines, %lld calls, %lld items\n", kFamily[f], n_lines[f], n_calls_made[f], n_items[f]);
    printf("searches: %lld, with tied lags %lld\n", searches, tied_searches);
    printf("ok %lld lines\n", n_lines[0] + n_lines[1] + n_lines[2] + n_lines[3]);
    return 0;
}
