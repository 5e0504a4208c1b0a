// The part of the shard core that makes no GPU call (spandsp_amd/csrc/shard_core.hpp), driven with made-up shard and channel
// counts: the dealing of the channels, range and info, and the two ways from a shard-major collecting slot back to the whole
// bank's channel order.  A program of its own, built with -fsanitize=address,undefined (tests/test_shard_core.py); it checks
// itself and exits non-zero on a miss.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "shard_core.hpp"

extern "C" int spangpu_set_error(int code, const char *) { return code; }

using namespace spg;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "shard_deal: %s fails at %d shards, %d channels (line %d)\n", #x, n, n_ch, __LINE__); exit(1); } } while (0)

static long check(int n, int n_ch)
{
    static ShardCore c;
    int devices[kMaxShards];
    for (int i = 0;  i < n;  i++)
        devices[i] = i % 8;
    c = ShardCore();
    CHECK(shard_deal(&c, devices, n, n_ch) == SPANGPU_OK);
    CHECK(c.n == n  &&  c.n_ch == n_ch  &&  c.collect_device == 0  &&  c.first[0] == 0  &&  c.first[n] == n_ch);
    int sum = 0;
    for (int i = 0;  i < n;  i++)
    {
        int device, first, count;
        spangpu_shard_info_t info;
        c.link[i] = (i == 0)  ?  SPANGPU_LINK_SAME  :  SPANGPU_LINK_PEER;
        CHECK(shard_range(&c, i, &device, &first, &count) == SPANGPU_OK  &&  shard_info(&c, i, 1, &info) == SPANGPU_OK);
        CHECK(device == i % 8  &&  info.device == device  &&  info.first_channel == first  &&  info.n_channels == count);
        CHECK(info.collect_device == 0  &&  info.link == c.link[i]  &&  info.forced_peer_copy == 1);
        CHECK(first == sum);                            // contiguous
        CHECK(count >= 1);
        // whole waves, until what is left (the shards behind keep a channel each) no longer holds one
        if (i < n - 1  &&  n_ch - first - (n - 1 - i) >= 64)
            CHECK(count % 64 == 0);
        sum += count;
    }
    CHECK(sum == n_ch);
    CHECK(shard_range(&c, n, nullptr, nullptr, nullptr) == SPANGPU_ERR_BAD_ARG  &&  shard_range(&c, -1, nullptr, nullptr, nullptr) == SPANGPU_ERR_BAD_ARG);
    CHECK(shard_info(&c, n, 0, nullptr) == SPANGPU_ERR_BAD_ARG  &&  shard_info(nullptr, 0, 0, nullptr) == SPANGPU_ERR_BAD_ARG);
    CHECK(shard_bank(&c, n) == nullptr  &&  shard_bank(nullptr, 0) == nullptr);
    // rows: 3 of the 5 rows a slot has room for; byte = f(row, channel)
    const int slot_rows = 5, rows = 3;
    std::vector<uint8_t> slot((size_t) slot_rows*n_ch, 0xEE), out((size_t) rows*n_ch, 0xDD);
    for (int i = 0;  i < n;  i++)
    {
        const int mine = shard_channels(&c, i);
        for (int r = 0;  r < rows;  r++)
            for (int k = 0;  k < mine;  k++)
                slot[(size_t) slot_rows*c.first[i] + (size_t) r*mine + k] = (uint8_t) (r*31 + (c.first[i] + k)*7);
    }
    shard_rows_to_channels(&c, slot.data(), slot_rows, rows, out.data());
    for (int r = 0;  r < rows;  r++)
        for (int ch = 0;  ch < n_ch;  ch++)
            CHECK(out[(size_t) r*n_ch + ch] == (uint8_t) (r*31 + ch*7));
    // blocks: 4 head bytes and 6 tail bytes a channel
    const size_t head = 4, tail = 6;
    std::vector<uint8_t> blocks((head + tail)*n_ch), heads(head*n_ch, 0xDD), tails(tail*n_ch, 0xDD);
    for (int i = 0;  i < n;  i++)
    {
        const size_t mine = (size_t) shard_channels(&c, i);
        uint8_t *blk = blocks.data() + (head + tail)*c.first[i];
        for (size_t k = 0;  k < mine*head;  k++)
            blk[k] = (uint8_t) ((head*c.first[i] + k)*3);
        for (size_t k = 0;  k < mine*tail;  k++)
            blk[mine*head + k] = (uint8_t) ((tail*c.first[i] + k)*5 + 1);
    }
    shard_blocks_to_channels(&c, blocks.data(), head, tail, heads.data(), tails.data());
    for (size_t k = 0;  k < head*n_ch;  k++)
        CHECK(heads[k] == (uint8_t) (k*3));
    for (size_t k = 0;  k < tail*n_ch;  k++)
        CHECK(tails[k] == (uint8_t) (k*5 + 1));
    return 1;
}

int main(void)
{
    long cases = 0;
    for (int n = 1;  n <= kMaxShards;  n++)
    {
        for (int n_ch = n;  n_ch <= n + 4200;  n_ch += (n_ch < n + 200)  ?  1  :  97)
            cases += check(n, n_ch);
    }
    // 200 channels over 3 shards: 128, 64 and 8
    static ShardCore c;
    const int devices[3] = {0, 0, 0};
    const int n = 3, n_ch = 200;
    CHECK(shard_deal(&c, devices, n, n_ch) == SPANGPU_OK);
    CHECK(c.first[0] == 0  &&  c.first[1] == 128  &&  c.first[2] == 192  &&  c.first[3] == 200);
    CHECK(shard_deal(&c, devices, 3, 2) == SPANGPU_ERR_BAD_ARG  &&  shard_deal(&c, devices, 0, 2) == SPANGPU_ERR_BAD_ARG
          &&  shard_deal(&c, devices, kMaxShards + 1, 1000) == SPANGPU_ERR_BAD_ARG);
    printf("shard_deal: %ld cases: ok\n", cases + 1);
    return 0;
}
