// tone_cadence.hpp -- super-tone cadences on the device (cadence_dev.hpp has the walk): the matcher a bank carries once
// spangpu_bank_set_cadences() gave it a set, and what the other tone units ask of tone_cadence.hip.  Host only.

#pragma once

#include "tone_bank.hpp"
#include "cadence_dev.hpp"

struct Cadence
{
    int n_tones;
    int n_elems;
    int tone_len[spg::kCadLdsTones + 1];    // elements of each of the first tones (host copy: spangpu_bank_cadence_set_state)
    int32_t *d_first;       // [n_tones + 1]
    int4 *d_elem;           // (pair, least blocks, most blocks, 0)
    int32_t *d_state;       // [kCadWords][n_ch]
    uint32_t *d_ev;         // [slots][n_ch][2]
    int32_t *d_count;       // [n_ch]
    uint32_t *h_ev;         // pinned
    int32_t *h_count;
    uint32_t *d_list;       // [2 + 3*slots_cap*n_ch]: two counters used in turn (a launch clears the next one's), then
                            // (channel, word 0, word 1) per event, a channel's together
    int which;              // the counter of the last launch
    uint32_t *h_list;       // pinned
    int slots_cap;
    int segments;
    unsigned done_serial;   // the launch whose records were matched last
    int last_slots;
    bool fused;             // the last detector launch matched the cadences itself (tone_fast.hpp, kToneCadence)
    bool list_due;          // ... and the compact list of its events has not been made yet
};

void cadence_free(Cadence *c);

// (the two below are on every launch's path: in the header, so that the launch unit has them inline)
static inline void cadence_args(const spangpu_bank_s *b, const Cadence *c, spg::CadenceArgs &A, int which)
{
    A.first = c->d_first;
    A.elem = c->d_elem;
    A.state = c->d_state;
    A.ev = c->d_ev;
    A.count = c->d_count;
    A.list = c->d_list;
    A.list_cap = (uint32_t) ((size_t) c->slots_cap*b->c.n_ch);
    A.n_tones = c->n_tones;
    A.segments = c->segments;
    A.which = which;
    A.n_elems = c->n_elems;
}

// A launch is about to overwrite the block records of the one before it.  If cadences are installed and nobody has taken
// that launch's records to the matcher yet (it was not served by the streaming kernel, and the caller did not ask for its
// cadence events), do it now: whether a bank's runs are counted must not depend on which kernel its frames happen to get.
static inline int cadence_catch_up(spangpu_bank_t *b)
{
    if (b->cad == nullptr  ||  b->launch_serial == 0  ||  b->cad->done_serial == b->launch_serial)
        return SPANGPU_OK;
    const int rc = spangpu_bank_cadence_run(b);
    return (rc < 0)  ?  rc  :  SPANGPU_OK;
}
