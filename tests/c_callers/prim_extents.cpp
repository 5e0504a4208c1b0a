// The staging rule of the fourteen spangpu_*_batch() primitives (spandsp_amd/csrc/prim_stage.hpp: which strides a call
// accepts, how many elements of an array it touches) and the table of their arguments, driven on the host: the header makes
// no GPU call, and prim_api.hip / prim2_api.hip take every staging and copy-back count from it.  A program of its own, built
// with -fsanitize=address,undefined (tests/test_prim_extents.py); it checks itself and exits non-zero on a miss.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "prim_stage.hpp"

using namespace spg;

#define CHECK(x, ...) do { if (!(x)) { fprintf(stderr, "prim_extents: %s fails (line %d): ", #x, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// ---- the rule against the indices the kernels form: base i*stride, element k of the row ------------------------------------
static long sweep(void)
{
    long cases = 0;
    for (int share = 0;  share < 2;  share++)
    for (int written = 0;  written < 2;  written++)
    for (int items = 1;  items <= 6;  items++)
    for (int row = 0;  row <= 6;  row++)
    for (int stride = 0;  stride <= 9;  stride++)
    {
        const bool allowed = (stride == 0)  ?  (share  &&  !written)  :  (stride >= row);
        long long top = -1;
        for (int i = 0;  i < items;  i++)
            for (int k = 0;  k < row;  k++)
                top = (i*stride + k > top)  ?  i*stride + k  :  top;
        size_t extent = 12345;
        const bool ok = prim_extent(row, stride, items, share, written, 4, &extent);
        CHECK(ok == allowed, "share %d written %d items %d row %d stride %d", share, written, items, row, stride);
        if (ok)
            CHECK(extent == (size_t) (top + 1), "extent %zu, the kernels reach %lld: items %d row %d stride %d", extent, top, items, row, stride);
        else
            CHECK(extent == 0, "a refusal leaves an extent of %zu", extent);
        // a written array's rows never overlap
        if (ok  &&  written  &&  items > 1)
            CHECK(stride >= row, "rows overlap");
        cases++;
    }
    for (int stride = -3;  stride < 0;  stride++)
    {
        size_t extent;
        CHECK(!prim_extent(4, stride, 3, true, false, 4, &extent)  &&  !prim_extent(0, stride, 1, true, false, 4, &extent), "stride %d", stride);
        cases++;
    }
    return cases;
}

// ---- nothing overflows: refused, and UBSan stays quiet -----------------------------------------------------------------
static long overflow(void)
{
    size_t e;
    const size_t elems[] = {1, 2, 4, 8};
    long cases = 0;
    for (size_t elem : elems)
    {
        const size_t most = SIZE_MAX/elem;
        CHECK(!prim_extent(1, LLONG_MAX, INT_MAX, true, false, elem, &e), "elem %zu", elem);
        CHECK(!prim_extent(1, LLONG_MAX, 4, false, true, elem, &e), "elem %zu", elem);
        CHECK(prim_extent(INT_MAX, LLONG_MAX - 1, 2, true, false, elem, &e) == (elem == 1), "elem %zu", elem);     // 2^63 + 2^31 - 2 elements
        CHECK(!prim_extent(LLONG_MAX, LLONG_MAX, 3, true, false, elem, &e), "elem %zu", elem);
        CHECK(!prim_extent(8, (long long) (most/2), 4, true, false, elem, &e), "elem %zu", elem);
        CHECK(!prim_extent(LLONG_MIN, 1, 1, true, false, elem, &e)  &&  !prim_extent(1, LLONG_MIN, 2, true, false, elem, &e), "elem %zu", elem);
        CHECK(!prim_extent(1, 1, 0, true, false, elem, &e)  &&  !prim_extent(1, 1, INT_MIN, true, false, elem, &e), "elem %zu", elem);
        // the largest that fits, exactly, and one more
        const size_t m = (size_t) INT_MAX - 1;
        const size_t s = (most - 7)/m;
        CHECK(s <= (size_t) LLONG_MAX, "stride");
        CHECK(prim_extent(7, (long long) s, INT_MAX, true, false, elem, &e)  &&  e == s*m + 7  &&  e <= most, "elem %zu", elem);
        if (s < (size_t) LLONG_MAX)
            CHECK(!prim_extent(7, (long long) s + 1, INT_MAX, true, false, elem, &e), "elem %zu", elem);
        // one item: the stride does not enter the extent, however long
        CHECK(prim_extent(5, LLONG_MAX, 1, false, true, elem, &e)  &&  e == 5, "elem %zu", elem);
        // a shared row: items do not enter it
        CHECK(prim_extent(5, 0, INT_MAX, true, false, elem, &e)  &&  e == 5, "elem %zu", elem);
        cases += 12;
    }
    CHECK(!prim_extent(1, 1, 1, false, false, 0, &e), "element size 0");
    // the table's back-to-back arrays at absurd sizes: dds out is [items][n] complex
    CHECK(!prim_arg_extent(kDdsOut, 0, INT_MAX, INT_MAX, &e), "dds out");
    CHECK(prim_arg_extent(kDdsOut, 0, INT_MAX, 1, &e)  &&  e == (size_t) INT_MAX, "dds out");
    CHECK(!prim_arg_extent(kVecLmsY, LLONG_MAX, INT_MAX, 27, &e)  &&  !prim_arg_extent(kPowerAmp, LLONG_MAX/2, 3, 160, &e), "strided");
    return cases + 5;
}

// ---- the table: what the calls' prototypes (include/spangpu.h) and, for one item, spandsp's own promise ---------------------
// row: elements of one item's row, of the element size beside it; by name (one item) that is the whole array:
//   vec_circular_dot_prodf(const float x[], const float y[], int n, int pos)          x[n], y[n]
//   cvec_circular_dot_prodf(const complexf_t x[], const complexf_t y[], int n, ...)   x[n], y[n] complex
//   *_lmsf(x, y, n, pos, error)                                                       x[n], y[n] (y updated)
//   power_meter_update(s, amp) a sample at a time                                     amp[n]
//   godard_ted_rx(s, sample) a sample at a time; the state and descriptor structs     samples[n], 8 words, 12 words
//   periodogram(const complexf_t coeffs[], const complexf_t amp[], int len)           coeffs[len/2], amp[len]
//   periodogram_prepare(sum, diff, amp, len)                                          sum[len/2], diff[len/2], amp[len]
//   periodogram_apply(coeffs, sum, diff, len)                                         coeffs[len/2], sum[len/2], diff[len/2]
//   dds_complexf(&acc, rate) n times                                                  n phasors
static long long one(int) { return 1; }
static long long whole(int n) { return n; }
static long long half(int n) { return n/2; }
static long long state_words(int) { return 8; }
static long long desc_words(int) { return 12; }

struct Promise
{
    const char *call;
    const char *name;
    long long (*row)(int);
    unsigned elem;
    bool may_share;
    bool written;
    bool strided;
};

static const Promise promises[] = {
    {"vec_circular_dot_prodf", "x", whole, 4, true, false, true},
    {"vec_circular_dot_prodf", "y", whole, 4, true, false, true},
    {"vec_circular_dot_prodf", "pos", one, 4, false, false, false},
    {"vec_circular_dot_prodf", "z", one, 4, false, true, false},
    {"vec_circular_lmsf", "x", whole, 4, true, false, true},
    {"vec_circular_lmsf", "y", whole, 4, false, true, true},
    {"vec_circular_lmsf", "pos", one, 4, false, false, false},
    {"vec_circular_lmsf", "error", one, 4, false, false, false},
    {"cvec_circular_dot_prodf", "x", whole, 8, true, false, true},
    {"cvec_circular_dot_prodf", "y", whole, 8, true, false, true},
    {"cvec_circular_dot_prodf", "pos", one, 4, false, false, false},
    {"cvec_circular_dot_prodf", "z", one, 8, false, true, false},
    {"cvec_circular_lmsf", "x", whole, 8, true, false, true},
    {"cvec_circular_lmsf", "y", whole, 8, false, true, true},
    {"cvec_circular_lmsf", "pos", one, 4, false, false, false},
    {"cvec_circular_lmsf", "error", one, 8, false, false, false},
    {"power_meter_update", "amp", whole, 2, true, false, true},
    {"power_meter_update", "reading", one, 4, false, true, false},
    {"power_meter_update", "shift", one, 4, false, false, false},
    {"godard_ted_rx", "state", state_words, 4, false, true, false},
    {"godard_ted_rx", "desc", desc_words, 4, true, false, true},
    {"godard_ted_rx", "samples", whole, 4, true, false, true},
    {"godard_ted_per_baud", "state", state_words, 4, false, true, false},
    {"godard_ted_per_baud", "desc", desc_words, 4, true, false, true},
    {"godard_ted_per_baud", "correction", one, 4, false, true, false},
    {"periodogram", "coeffs", half, 8, true, false, true},
    {"periodogram", "amp", whole, 8, true, false, true},
    {"periodogram", "out", one, 8, false, true, false},
    {"periodogram_prepare", "amp", whole, 8, true, false, true},
    {"periodogram_prepare", "sum", half, 8, false, true, false},
    {"periodogram_prepare", "diff", half, 8, false, true, false},
    {"periodogram_apply", "coeffs", half, 8, true, false, true},
    {"periodogram_apply", "sum", half, 8, false, false, false},
    {"periodogram_apply", "diff", half, 8, false, false, false},
    {"periodogram_apply", "out", one, 8, false, true, false},
    {"periodogram_freq_error", "last_result", one, 8, false, false, false},
    {"periodogram_freq_error", "result", one, 8, false, false, false},
    {"periodogram_freq_error", "out", one, 4, false, true, false},
    {"fixed_sqrt32", "x", one, 4, false, false, false},
    {"fixed_sqrt32", "out", one, 2, false, true, false},
    {"dds_complexf", "phase_acc", one, 4, false, true, false},
    {"dds_complexf", "phase_rate", one, 4, false, false, false},
    {"dds_complexf", "out", whole, 8, false, true, false},
    {"arctan2", "y", one, 4, false, false, false},
    {"arctan2", "x", one, 4, false, false, false},
    {"arctan2", "out", one, 4, false, true, false},
};

static long table(void)
{
    const int n_promises = (int) (sizeof(promises)/sizeof(promises[0]));
    CHECK(kPrimArgCount == n_promises, "%d arguments in the table, %d promised", kPrimArgCount, n_promises);
    int calls = 0;
    long cases = 0;
    for (int j = 0;  j < n_promises;  j++)
    {
        const Promise &p = promises[j];
        const PrimArg &a = kPrimArgs[j];
        if (j == 0  ||  strcmp(p.call, promises[j - 1].call) != 0)
            calls++;
        CHECK(strcmp(a.call, p.call) == 0  &&  strcmp(a.name, p.name) == 0, "entry %d is %s.%s, not %s.%s", j, a.call, a.name, p.call, p.name);
        CHECK(a.elem == p.elem  &&  a.may_share == p.may_share  &&  (a.use != kIn) == p.written  &&  a.strided == p.strided, "%s.%s", p.call, p.name);
        CHECK(!(a.may_share  &&  a.use != kIn)  &&  (a.strided  ||  !a.may_share), "%s.%s: a written or back-to-back array is never shared", p.call, p.name);
        for (int n = 1;  n <= 40;  n++)
        {
            const long long row = p.row(n);
            size_t e = 99;
            CHECK(prim_row(a.row, n) == row, "%s.%s: a row of %lld at n = %d", p.call, p.name, prim_row(a.row, n), n);
            // the by-name shims' shape: one item, stride 0 where a row may be shared, else the row itself
            if (a.may_share)
            {
                CHECK(prim_arg_extent(a, 0, 1, n, &e)  &&  e == (size_t) row, "%s.%s[%lld] at n = %d, one item, stride 0: %zu", p.call, p.name, row, n, e);
                CHECK(prim_arg_extent(a, 0, 300, n, &e)  &&  e == (size_t) row, "%s.%s shared by 300 items: %zu", p.call, p.name, e);
            }
            else if (a.strided)
            {
                CHECK(!prim_arg_extent(a, 0, 1, n, &e)  &&  !prim_arg_extent(a, 0, 5, n, &e), "%s.%s takes a stride of 0", p.call, p.name);
            }
            if (row > 0)
                CHECK(prim_arg_extent(a, row, 1, n, &e)  &&  e == (size_t) row, "%s.%s[%lld] at n = %d, one item: %zu", p.call, p.name, row, n, e);
            if (a.strided)
            {
                CHECK(prim_arg_extent(a, row + 3, 5, n, &e)  &&  e == (size_t) ((row + 3)*4 + row)*(row > 0), "%s.%s padded: %zu", p.call, p.name, e);
                CHECK(!prim_arg_extent(a, -1, 5, n, &e)  &&  !prim_arg_extent(a, -row - 1, 1, n, &e), "%s.%s takes a negative stride", p.call, p.name);
                if (row > 1)
                    CHECK(!prim_arg_extent(a, row - 1, 5, n, &e)  &&  !prim_arg_extent(a, row - 1, 1, n, &e), "%s.%s takes a stride of row - 1", p.call, p.name);
            }
            else
            {
                // back to back, whatever the stride argument says
                CHECK(prim_arg_extent(a, 0, 5, n, &e)  &&  e == (size_t) (5*row), "%s.%s back to back: %zu", p.call, p.name, e);
                CHECK(prim_arg_extent(a, -77, 5, n, &e)  &&  e == (size_t) (5*row), "%s.%s back to back: %zu", p.call, p.name, e);
            }
            cases++;
        }
    }
    CHECK(calls == 14, "%d calls in the table", calls);
    // in particular: periodogram's coefficients are len/2 complex, none for len 1 (and the call is accepted)
    size_t e = 99;
    CHECK(prim_arg_extent(kPgramCoeffs, 0, 1, 33, &e)  &&  e == 16, "coeffs[len/2]: %zu", e);
    CHECK(prim_arg_extent(kPgramCoeffs, 0, 1, 2, &e)  &&  e == 1, "coeffs[len/2]: %zu", e);
    CHECK(prim_arg_extent(kPgramCoeffs, 0, 7, 1, &e)  &&  e == 0, "len 1: %zu", e);
    // the power meter's shared row is a row, not stride*items = 0 samples
    CHECK(prim_arg_extent(kPowerAmp, 0, 257, 160, &e)  &&  e == 160, "power meter, shared: %zu", e);
    return cases + 4;
}

int main(void)
{
    long cases = sweep();
    cases += overflow();
    cases += table();
    printf("%ld cases: ok\n", cases);
    return 0;
}
