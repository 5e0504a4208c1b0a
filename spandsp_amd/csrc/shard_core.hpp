// shard_core.hpp -- what the three sets of banks over several devices share (shard_api.hip: spangpu_shard_*, spangpu_echo_shard_*,
// spangpu_modem_shard_*): which device has which channels, the banks, every shard's result buffer, the two collecting slots
// and their events.  This header is the part without a GPU call in it -- the dealing of the channels, range, info and the way
// back to the whole bank's channel order on the host -- so that a program of its own can drive it
// (tests/c_callers/shard_deal.cpp); the calls that touch a device are in shard_api.hip.  Nothing here is exported.

#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include "../../include/spangpu.h"

extern "C" int spangpu_set_error(int code, const char *msg);

namespace spg __attribute__((visibility("hidden")))
{

enum { kMaxShards = 64 };

// the three calls of a bank type the core makes
struct ShardOps
{
    int (*sync)(void *bank);
    int (*destroy)(void *bank);
    void *(*get_stream)(void *bank);
};

struct ShardCore
{
    const ShardOps *ops;
    int n;                              // shards
    int n_ch;                           // channels of the whole bank
    int collect_device;                 // where the gathered bytes go: the first shard's device
    int device[kMaxShards];
    int first[kMaxShards + 1];          // first channel of shard i; first[n] = n_ch
    int link[kMaxShards];               // SPANGPU_LINK_*: how shard i's bytes reach the collecting device
    void *bank[kMaxShards];
    void *out[kMaxShards];              // the shard's results of a step, on the shard's device
    hipEvent_t done[2][kMaxShards];     // the shard's bytes of a step have arrived on the collecting device (per slot)
    void *gathered[2];                  // on collect_device.  Two slots used in turn: a step's bytes stay whole while the next step
                                        // is queued and runs (a reader that takes a step's bytes before the step after next is
                                        // queued never sees a mix)
    void *h_gathered;                   // pinned host copy of a slot, for the families that reorder on the host
    unsigned steps;                     // steps (reports) queued so far; the last one wrote slot (steps - 1) & 1
};

static inline int shard_channels(const ShardCore *c, int i)
{
    return c->first[i + 1] - c->first[i];
}

// devices[i] is the HIP device of shard i (a device may appear more than once: two shards on one GPU, each with its own
// stream -- how a one-GPU box exercises this path).  Channels are dealt in contiguous ranges, as evenly as they go, in
// multiples of 64 (a wavefront's worth) until what is left only gives the shards behind a channel each; the last shard takes
// the rest.
static inline int shard_deal(ShardCore *c, const int *devices, int n_devices, int n_channels)
{
    if (n_devices < 1  ||  n_devices > kMaxShards  ||  n_channels < n_devices)
        return SPANGPU_ERR_BAD_ARG;
    c->n = n_devices;
    c->n_ch = n_channels;
    c->collect_device = devices[0];
    const int per = ((n_channels + n_devices - 1)/n_devices + 63)/64*64;
    int at = 0;
    for (int i = 0;  i < n_devices;  i++)
    {
        c->device[i] = devices[i];
        c->first[i] = at;
        const int left = n_channels - at;
        const int behind = n_devices - 1 - i;
        int mine = (per < left - behind)  ?  per  :  (left - behind);
        if (mine >= 64)
            mine &= ~63;
        if (mine < 1)
            mine = 1;
        if (behind == 0)
            mine = left;
        at += mine;
    }
    c->first[n_devices] = n_channels;
    return (at == n_channels)  ?  SPANGPU_OK  :  SPANGPU_ERR_BAD_ARG;
}

// Shard i: its device, its first channel and how many it has.
static inline int shard_range(const ShardCore *c, int i, int *device, int *first_channel, int *n_channels)
{
    if (c == nullptr  ||  i < 0  ||  i >= c->n)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad shard");
    if (device) *device = c->device[i];
    if (first_channel) *first_channel = c->first[i];
    if (n_channels) *n_channels = shard_channels(c, i);
    return SPANGPU_OK;
}

static inline int shard_info(const ShardCore *c, int i, int forced_peer_copy, spangpu_shard_info_t *info)
{
    if (c == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null shard set");
    if (i < 0  ||  i >= c->n  ||  info == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad shard");
    info->device = c->device[i];
    info->first_channel = c->first[i];
    info->n_channels = shard_channels(c, i);
    info->collect_device = c->collect_device;
    info->link = c->link[i];
    info->forced_peer_copy = forced_peer_copy;
    return SPANGPU_OK;
}

static inline void *shard_bank(const ShardCore *c, int i)
{
    return (c  &&  i >= 0  &&  i < c->n)  ?  c->bank[i]  :  nullptr;
}

// A gathered slot is shard-major.  Rows: shard i's bytes, [rows][its channels], stand at slot_rows*first[i];
// dst[r*n_ch + c] = row r of channel c.
static inline void shard_rows_to_channels(const ShardCore *c, const uint8_t *slot, int slot_rows, int rows, uint8_t *dst)
{
    for (int i = 0;  i < c->n;  i++)
    {
        const size_t mine = (size_t) shard_channels(c, i);
        const uint8_t *src = slot + (size_t) slot_rows*c->first[i];
        for (int r = 0;  r < rows;  r++)
            memcpy(dst + (size_t) r*c->n_ch + c->first[i], src + (size_t) r*mine, mine);
    }
}

// Blocks: shard i's block stands at (head + tail)*first[i] and holds head bytes for each of its channels, then tail bytes for
// each; the heads of all channels go to `heads`, the tails to `tails`, both in the whole bank's channel order.
static inline void shard_blocks_to_channels(const ShardCore *c, const uint8_t *slot, size_t head, size_t tail, uint8_t *heads, uint8_t *tails)
{
    for (int i = 0;  i < c->n;  i++)
    {
        const size_t mine = (size_t) shard_channels(c, i);
        const uint8_t *blk = slot + (head + tail)*c->first[i];
        memcpy(heads + head*c->first[i], blk, mine*head);
        memcpy(tails + tail*c->first[i], blk + mine*head, mine*tail);
    }
}

}   // namespace spg
