// tone_bank.hpp -- the tone bank on the host: its struct, and what its units call across (tone_api.hip: life, streams, read-backs;
// tone_rx.hip: the launch path; tone_state.hip: state and parameters; tone_cadence.hip: the cadence matcher).  Nothing exported.

#pragma once

#include "bank_host.hpp"

constexpr int kToneMaxBins = SPANGPU_MAX_BINS;      // = kMaxBins and
constexpr int kToneMaxMulti = 4;                    // = kMaxMulti of tone_dev.hpp, which only tone_rx.hip includes (and checks)

struct spangpu_bank_s
{
    spg::BankCore c;            // device, channel count, the bank's stream (st is unused: sf and si below are the state)
    int kind;
    bool timing;
    // Queue mode (spangpu_bank_set_queues(bank, 2)): the streaming kernel's launch is cut in two workgroup ranges, the second
    // on a stream (= hardware queue) of its own, so that one half's launch boundary, start burst and write-back lie under the
    // other half's steady state (profiles/r5_probe_mq.log).  ev_in orders the second stream behind whatever the bank's stream
    // held when the launch was queued; ev_q, recorded behind the second half, is what joined() makes the bank's stream wait for.
    int queues;
    hipStream_t stream2;
    hipEvent_t ev_in;
    hipEvent_t ev_q;
    bool s2_busy;               // the second stream holds launches the bank's stream has not been made to wait for
    bool main_touched;          // the bank's stream was handed out or used since the last split launch: the next one orders
                                // the second stream behind it.  (Between two split launches with nothing else in between
                                // NO event is recorded or waited for: the two queues run free, which is where the gain is --
                                // a wait per tick made 131 072 channels take 38 us a tick instead of 16.5.)
    spangpu_tone_params_t tp;
    // geometry of the detector
    int nb;                 // bins compiled into the kernel used
    int nsf;                // float state words per channel
    int block_len;
    float fac[kToneMaxBins];
    float threshold;
    float normal_twist;
    float reverse_twist;
    // device state
    float *sf;
    int32_t *si;
    // per-call outputs (capacity = maxb_cap blocks)
    int maxb_cap;
    uint32_t *rec;
    uint32_t *ext_rec;          // caller-owned record buffer for the next launches (spangpu_bank_set_records_buffer)
    size_t ext_rec_bytes;
    uint8_t *ext_digits;        // caller-owned digit bytes of the next launches (spangpu_bank_set_digits_buffer / _ring):
    size_t ext_digits_bytes;    // ... bytes per slice, slices, and which slice the next launch fills
    int ext_digits_slices;
    int ext_digits_next;
    uint32_t *cur_rec;          // where the last launch wrote its records
    int next_fmt;               // sample format of the launch being prepared (0 linear, 1 A-law, 2 u-law)
    spg::VarLens lens;          // per-channel lengths of the launch being prepared (lens.next), or nullptr
    bool next_ragged;           // ... some of them are neither 0 nor the longest
    float *chan_parms;          // DTMF, once a channel was given parameters of its own: [4][n_ch] on the device
    float *h_chan_parms;        // ... and its host mirror
    int n_filter_on;            // channels whose dial tone filter is on
    float *rec_energy;
    int32_t *rec_dur;
    float *trace;
    // host mirrors (pinned)
    uint32_t *h_rec;
    float *h_energy;
    int32_t *h_dur;
    // staging for host-resident frames
    int16_t *d_amp;
    size_t d_amp_cap;       // in samples
    // last call
    int last_maxb;
    int last_samples;
    unsigned launch_serial;     // counts launches (the cadence matcher takes each launch's records once)
    struct Cadence *cad;        // super-tone: the cadence matcher on the device (spangpu_bank_set_cadences; tone_cadence.hpp)
    hipEvent_t ev0;
    hipEvent_t ev1;
    bool ev_valid;
};

// The bank's stream, with the second queue's last launch joined into it if one is outstanding: every entry point that puts work
// on the stream, waits for it, or hands it out goes through here (the split launch itself excepted), and so does every call
// of the shared core's that uses c.stream.
static inline hipStream_t joined(spangpu_bank_s *b)
{
    if (b->s2_busy)
    {
        (void) hipEventRecord(b->ev_q, b->stream2);
        (void) hipStreamWaitEvent(b->c.stream, b->ev_q, 0);
        b->s2_busy = false;
    }
    b->main_touched = true;
    return b->c.stream;
}

// where the last launch wrote its records
static inline uint32_t *records_of(const spangpu_bank_s *b)
{
    return b->cur_rec  ?  b->cur_rec  :  b->rec;
}

int ensure_outputs(spangpu_bank_s *b, int maxb);
void free_outputs(spangpu_bank_s *b);                // tone_api.hip: the per-call output blocks, for launches of up to maxb blocks
// tone_state.hip: a DTMF bank's thresholds from its parameters
void dtmf_levels(const spangpu_tone_params_t &tp, float &threshold, float &normal_twist, float &reverse_twist);
