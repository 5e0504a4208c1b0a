// adsi_frame.hpp -- the message framers of the caller-ID (ADSI) banks, as plain functions over one channel's words:
// adsi_tx_get_bit() and adsi_rx_put_bit() of the reference (src/adsi.c:94-170, 192-328) with crc_itu16_calc() bit by bit
// (src/crc.c:161-169).  adsi_dev.hpp runs them behind the FSK modulator and demodulator; they compile for the host as they
// are (tests/c_callers/adsi_frame_host.cpp runs them one channel at a time beside the reference).

#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ADSI_HD __host__ __device__ __forceinline__
#define ADSI_HDN __host__ __device__ __noinline__
#else
#define ADSI_HD static inline
#define ADSI_HDN static inline
#endif

namespace spg
{

constexpr int kAdsiMsg = 256;               // uint8_t msg[256], either way
constexpr int kAdsiJclip = 4;               // ADSI_STANDARD_JCLIP
constexpr int kAdsiDle = 0x10;

// The message layer of one sender while a call runs
struct AdsiTx
{
    int preamble_len, preamble_ones_len, postamble_ones_len, stop_bits;
    int byte_no, bit_pos, bit_no, msg_len, signal_on;
    const uint8_t *msg;         // this channel's kAdsiMsg bytes
};

// adsi_tx_get_bit(): 0 or 1, or -1 for SIG_STATUS_END_OF_DATA
ADSI_HD int adsi_next_bit(AdsiTx &t)
{
    const int marks_end = t.preamble_len + t.preamble_ones_len;
    if (t.bit_no < t.preamble_len)
        return t.bit_no++ & 1;
    if (t.bit_no < marks_end)
    {
        t.bit_no++;
        return 1;
    }
    if (t.bit_no <= marks_end)
    {
        if (t.bit_pos == 0)
        {
            t.bit_pos++;
            return 0;
        }
        if (t.bit_pos < 1 + 8)
        {
            // (byte_no stays below msg_len, or is 0 for a sender nothing was put into)
            const int bit = (t.msg[t.byte_no & (kAdsiMsg - 1)] >> (t.bit_pos - 1)) & 1;
            t.bit_pos++;
            return bit;
        }
        if (t.bit_pos < 1 + 8 + t.stop_bits - 1)
        {
            t.bit_pos++;
            return 1;
        }
        t.bit_pos = 0;
        if (++t.byte_no >= t.msg_len)
            t.bit_no++;
        return 1;
    }
    if (t.bit_no <= marks_end + t.postamble_ones_len)
    {
        t.bit_no++;
        return 1;
    }
    if (t.signal_on)
    {
        t.signal_on = 0;
        t.msg_len = 0;
    }
    return -1;
}

// The framer of one receiver while a call runs: adsi_rx_put_bit() as the demodulator's put_bit
struct AdsiRx
{
    int standard, ones, bit_pos, in_progress, msg_len, framing_errors, count;
    uint8_t *msg;               // this channel's kAdsiMsg bytes
    uint8_t *rec_bytes;         // this channel's record
    int32_t *rec_lens;
    int cap;
};

// put_msg(user_data, msg, len): one more entry of the call's record
ADSI_HD void adsi_deliver(const uint8_t *msg, int len, uint8_t *rec_bytes, int32_t *rec_lens, int cap, int count)
{
    if (count < cap)
    {
        uint8_t *to = rec_bytes + (size_t) count*kAdsiMsg;
        for (int i = 0;  i < len;  i++)
            to[i] = msg[i];
        rec_lens[count] = len;
    }
}

// A whole byte with a good stop bit, adsi.c:256-316: returns the new msg_len, with bit 16 set when a message was delivered.
// Out of line and on values, so that the framer's words stay in registers: this runs once in ten bit times.
ADSI_HDN int adsi_put_byte(uint8_t *msg, int standard, int in_progress, int msg_len, uint8_t *rec_bytes, int32_t *rec_lens,
                                          int cap, int count)
{
    int delivered = 0;
    if (msg_len >= kAdsiMsg)
        return msg_len;
    if (standard == kAdsiJclip)
    {
        // a message starts DLE SOH; only the DLE, with its parity bit, is looked for
        if (msg_len != 0  ||  in_progress == (0x80 | kAdsiDle))
            msg[msg_len++] = (uint8_t) in_progress;
        if (msg_len >= 11  &&  msg_len == (msg[6] & 0x7F) + 11)
        {
            uint32_t crc = 0u;
            for (int i = 2;  i < msg_len;  i++)
            {
                crc ^= msg[i];
                for (int k = 0;  k < 8;  k++)
                    crc = (crc & 1u)  ?  ((crc >> 1) ^ 0x8408u)  :  (crc >> 1);
            }
            if (crc == 0u)
            {
                for (int i = 0;  i < msg_len - 2;  i++)
                    msg[i] &= 0x7F;
                adsi_deliver(msg, msg_len - 2, rec_bytes, rec_lens, cap, count);
                delivered = 0x10000;
            }
            msg_len = 0;
        }
    }
    else
    {
        msg[msg_len++] = (uint8_t) in_progress;
        if (msg_len >= 3  &&  msg_len == msg[1] + 3)
        {
            int sum = 0;
            for (int i = 0;  i < msg_len - 1;  i++)
                sum += msg[i];
            if ((-sum & 0xFF) == msg[msg_len - 1])
            {
                adsi_deliver(msg, msg_len - 1, rec_bytes, rec_lens, cap, count);
                delivered = 0x10000;
            }
            msg_len = 0;
        }
    }
    return msg_len | delivered;
}

ADSI_HD void adsi_put_bit(AdsiRx &v, int bit)
{
    if (bit < 0)
    {
        if (bit == -2)
        {
            // SIG_STATUS_CARRIER_UP
            v.ones = 0;
            v.bit_pos = 0;
            v.in_progress = 0;
            v.msg_len = 0;
        }
        return;
    }
    bit &= 1;
    if (v.bit_pos == 0)
    {
        if (bit == 0)
        {
            v.bit_pos = 1;
            // more than 10 marks ahead of a start bit: the line was idle, message acquisition starts again
            v.msg_len = (v.ones > 10)  ?  0  :  v.msg_len;
            v.ones = 0;
        }
        else
        {
            v.ones++;
        }
    }
    else if (v.bit_pos <= 8)
    {
        v.in_progress = (v.in_progress >> 1) | (bit  ?  0x80  :  0);
        v.bit_pos++;
    }
    else
    {
        if (bit)
        {
            const int r = adsi_put_byte(v.msg, v.standard, v.in_progress, v.msg_len, v.rec_bytes, v.rec_lens, v.cap, v.count);
            v.msg_len = r & 0xFFFF;
            v.count += r >> 16;
        }
        else
        {
            v.framing_errors++;
        }
        v.bit_pos = 0;
        v.in_progress = 0;
    }
}

}   // namespace spg
