// The parts of the receivers' shared host plumbing that make no GPU call (spandsp_amd/csrc/bank_host.hpp): the check of an
// _rx_var call's per-channel lengths and the scan of one row of result counts, driven with made-up lengths and counts over
// 1 .. 200 channels.  A program of its own, built with -fsanitize=address,undefined (tests/test_rx_core.py); it checks
// itself and exits non-zero on a miss.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "bank_host.hpp"

static int g_errors_set = 0;
extern "C" int spangpu_set_error(int code, const char *) { g_errors_set++; return code; }

using namespace spg;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "rx_core: %s fails at %d channels (line %d)\n", #x, n, __LINE__); exit(1); } } while (0)

static long check_lens(int n)
{
    const int max_samples = 160;
    int longest = -7;
    bool all = false;
    std::vector<int32_t> lens(n, 0);
    // nobody, everybody the same, everybody the most
    CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_OK  &&  longest == 0  &&  all);
    lens.assign(n, 37);
    CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_OK  &&  longest == 37  &&  all);
    lens.assign(n, max_samples);
    CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_OK  &&  longest == max_samples  &&  all);
    // one channel apart, at the first, a middle and the last channel: shorter, longer, and out of range either way
    const int where[3] = {0, n/2, n - 1};
    for (int w = 0;  w < 3;  w++)
    {
        lens.assign(n, 37);
        lens[where[w]] = 0;
        CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_OK  &&  longest == ((n == 1)  ?  0  :  37)  &&  all == (n == 1));
        lens[where[w]] = max_samples;
        CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_OK  &&  longest == max_samples  &&  all == (n == 1));
        const int before = g_errors_set;
        lens[where[w]] = -1;
        CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_ERR_BAD_ARG);
        lens[where[w]] = max_samples + 1;
        CHECK(lens_check(lens.data(), n, max_samples, &longest, &all) == SPANGPU_ERR_BAD_ARG);
        CHECK(g_errors_set == before + 2);
    }
    // max_samples 0 (the modem bank's empty tick): zeros pass, a sample does not
    lens.assign(n, 0);
    CHECK(lens_check(lens.data(), n, 0, &longest, &all) == SPANGPU_OK  &&  longest == 0  &&  all);
    lens[n - 1] = 1;
    CHECK(lens_check(lens.data(), n, 0, &longest, &all) == SPANGPU_ERR_BAD_ARG);
    return 1;
}

static long check_counts(int n)
{
    const int cap = 12;
    int most = -7;
    std::vector<int32_t> row(n, 0);
    CHECK(count_row_scan(row.data(), n, cap, &most)  &&  most == 0);
    CHECK(count_row_scan(row.data(), n, 0, &most)  &&  most == 0);            // (a row that only says "did not fit")
    const int where[3] = {0, n/2, n - 1};
    for (int w = 0;  w < 3;  w++)
    {
        row.assign(n, 3);
        row[where[w]] = cap - 1;
        CHECK(count_row_scan(row.data(), n, cap, &most)  &&  most == cap - 1);
        row[where[w]] = cap;
        CHECK(count_row_scan(row.data(), n, cap, &most)  &&  most == cap);
        row[where[w]] = cap + 1;
        CHECK(!count_row_scan(row.data(), n, cap, &most)  &&  most == cap + 1);
        row.assign(n, 0);
        row[where[w]] = 1;
        CHECK(count_row_scan(row.data(), n, cap, &most)  &&  most == 1  &&  !count_row_scan(row.data(), n, 0, &most));
    }
    return 1;
}

int main(void)
{
    long cases = 0;
    for (int n = 1;  n <= 200;  n++)
        cases += check_lens(n) + check_counts(n);
    printf("rx_core: %ld cases: ok\n", cases);
    return 0;
}
