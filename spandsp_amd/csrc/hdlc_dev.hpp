// hdlc_dev.hpp -- HDLC framing banks: one lane per channel runs the reference's hdlc_rx_put_bit() / hdlc_rx_put_byte() over a
// row of a receiver bank's events, or hdlc_tx_get_bit() into a row of bits for a sender bank's ring (src/hdlc.c, src/crc.c of
// the reference).  All integer.  The per-channel step functions are plain inline functions over a channel's words in
// registers (int32_t w[]), its 404-byte frame buffer behind a one-word cache (HdlcBuf) and a sink for what the reference
// hands to its handlers; they compile for the host as they are (tests/c_callers/hdlc_host.cpp runs them one lane at a time).
//
// State is st[word][n_ch]; the frame buffer is buf[101][n_ch] 32-bit words, octet p in bits 8*(p & 3) of word p >> 2.  A lane
// gathers four octets in the cached word and stores it when it moves on, so lanes at the same position store side by side.
// The 404 bytes are never cleared: the reference's are not, and a frame reported bad after its length was forced past the
// buffer shows what earlier frames left there.

#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HDLC_HD __host__ __device__ __forceinline__
#define HDLC_HDM __host__ __device__ __forceinline__
#else
#define HDLC_HD static inline
#define HDLC_HDM inline
#endif

namespace spg
{

constexpr int kHdlcMaxFrame = 400;          // HDLC_MAXFRAME_LEN
constexpr int kHdlcBuf = 404;               // sizeof(buffer): the frame and a CRC-32
constexpr int kHdlcBufWords = 101;

// SIG_STATUS_* (spandsp/async.h)
constexpr int kSigCarrierDown = -1;
constexpr int kSigCarrierUp = -2;
constexpr int kSigTrainingInProgress = -3;
constexpr int kSigTrainingSucceeded = -4;
constexpr int kSigTrainingFailed = -5;
constexpr int kSigFramingOk = -6;
constexpr int kSigEndOfData = -7;
constexpr int kSigAbort = -8;
constexpr int kSigOctetReport = -11;

// hdlc_rx_state_t, in the order of its fields
enum
{
    HR_CRC_BYTES = 0,
    HR_MAX_FRAME_LEN,
    HR_REPORT_BAD_FRAMES,
    HR_FRAMING_OK_THRESHOLD,
    HR_FRAMING_OK_ANNOUNCED,
    HR_FLAGS_SEEN,
    HR_RAW_BIT_STREAM,
    HR_BYTE_IN_PROGRESS,
    HR_NUM_BITS,
    HR_OCTET_COUNTING_MODE,
    HR_OCTET_COUNT,
    HR_OCTET_COUNT_REPORT_INTERVAL,
    HR_LEN,
    HR_RX_BYTES,
    HR_RX_FRAMES,
    HR_RX_CRC_ERRORS,
    HR_RX_LENGTH_ERRORS,
    HR_RX_ABORTS,
    kHdlcRxWords
};

// hdlc_tx_state_t, in the order of its fields; then the command queue's read slot and fill
enum
{
    HT_CRC_BYTES = 0,
    HT_INTER_FRAME_FLAGS,
    HT_PROGRESSIVE,
    HT_MAX_FRAME_LEN,
    HT_OCTETS_IN_PROGRESS,
    HT_NUM_BITS,
    HT_IDLE_OCTET,
    HT_FLAG_OCTETS,
    HT_ABORT_OCTETS,
    HT_REPORT_FLAG_UNDERFLOW,
    HT_LEN,
    HT_POS,
    HT_CRC,
    HT_BYTE,
    HT_BITS,
    HT_TX_END,
    kHdlcTxRefWords,
    HT_Q_HEAD = kHdlcTxRefWords,
    HT_Q_COUNT,
    kHdlcTxWords
};

// A queue slot's header word: the command in bits 0..2, "corrupt" in bit 3, the frame length or the flag count from bit 8 up
// (signed).  Its 404 bytes follow in a block of their own.
enum
{
    kHdlcCmdFrame = 1,
    kHdlcCmdFlags = 2,
    kHdlcCmdAbort = 3,
    kHdlcCmdEnd = 4
};
constexpr int kHdlcCmdCorrupt = 8;

// ---- the frame buffer of one channel ---------------------------------------------------------------------------------

struct HdlcBuf
{
    uint32_t *base;         // word 0 of this channel
    size_t stride;          // words between consecutive words of the channel (n_ch; 1 on the host)
    int at;                 // the cached word's index, -1: none
    uint32_t word;
    bool dirty;

    HDLC_HDM void open(uint32_t *b, size_t s)
    {
        base = b;
        stride = s;
        at = -1;
        word = 0;
        dirty = false;
    }

    HDLC_HDM void seek(int w)
    {
        if (w == at)
            return;
        if (dirty)
            base[(size_t) at*stride] = word;
        word = base[(size_t) w*stride];
        at = w;
        dirty = false;
    }

    HDLC_HDM int get(int pos)
    {
        seek(pos >> 2);
        return (int) ((word >> (8*(pos & 3))) & 0xFFu);
    }

    HDLC_HDM void put(int pos, int octet)
    {
        seek(pos >> 2);
        const int sh = 8*(pos & 3);
        word = (word & ~(0xFFu << sh)) | ((uint32_t) (octet & 0xFF) << sh);
        dirty = true;
    }

    HDLC_HDM void close()
    {
        if (dirty)
            base[(size_t) at*stride] = word;
        dirty = false;
    }
};

// crc_itu16_calc() / crc_itu32_calc() one octet on, in the shift and xor form (a table would be indexed per lane)
HDLC_HD uint32_t hdlc_crc_octet(uint32_t crc, int octet, int crc_bytes)
{
    const uint32_t poly = (crc_bytes == 2)  ?  0x8408u  :  0xEDB88320u;
    crc ^= (uint32_t) octet;
    for (int i = 0;  i < 8;  i++)
        crc = (crc >> 1) ^ (poly & (0u - (crc & 1u)));
    return crc;
}

// ---- receiver --------------------------------------------------------------------------------------------------------

// What the handlers of one channel saw in one call: recs[] in call order (>= 0: a frame, len | ok << 16; < 0: a status), the
// frames' octets back to back in bytes[].  n_recs and n_bytes go on counting past the capacities; nothing is written there.
struct HdlcRxSink
{
    int32_t *recs;
    uint8_t *bytes;
    int rec_cap;
    int byte_cap;
    int n_recs;
    int n_bytes;

    HDLC_HDM void status(int code)
    {
        if (n_recs < rec_cap)
            recs[n_recs] = code;
        n_recs++;
    }

    HDLC_HDM void frame(HdlcBuf &buf, int len, bool ok)
    {
        if (n_recs < rec_cap)
            recs[n_recs] = len | (ok  ?  0x10000  :  0);
        n_recs++;
        // (len can be 405 - crc_bytes: the buffer has 404 octets, and the reference's handler is handed that length of it)
        if (n_bytes + len <= byte_cap)
        {
            for (int i = 0;  i < len;  i++)
                bytes[n_bytes + i] = (uint8_t) ((i < kHdlcBuf)  ?  buf.get(i)  :  0);
        }
        n_bytes += len;
    }
};

// octet_set_and_count() (start == true) and octet_count()
HDLC_HD void hdlc_rx_octet_count(int32_t *w, HdlcRxSink &out, bool start)
{
    if (w[HR_OCTET_COUNT_REPORT_INTERVAL] == 0)
        return;
    if (w[HR_OCTET_COUNTING_MODE])
    {
        if (--w[HR_OCTET_COUNT] <= 0)
        {
            w[HR_OCTET_COUNT] = w[HR_OCTET_COUNT_REPORT_INTERVAL];
            out.status(kSigOctetReport);
        }
    }
    else if (start)
    {
        w[HR_OCTET_COUNTING_MODE] = 1;
        w[HR_OCTET_COUNT] = w[HR_OCTET_COUNT_REPORT_INTERVAL];
    }
}

HDLC_HD bool hdlc_rx_crc_good(const int32_t *w, HdlcBuf &buf)
{
    const int crc_bytes = w[HR_CRC_BYTES];
    uint32_t crc = (crc_bytes == 2)  ?  0xFFFFu  :  0xFFFFFFFFu;
    for (int i = 0;  i < w[HR_LEN];  i++)
        crc = hdlc_crc_octet(crc, buf.get(i), crc_bytes);
    return (crc_bytes == 2)  ?  ((crc & 0xFFFFu) == 0xF0B8u)  :  (crc == 0xDEBB20E3u);
}

// Back off after an abort, a misplaced flag or an over-long frame: to nothing before framing was nearly there, else to one
// flag short of it.
HDLC_HD void hdlc_rx_back_off(int32_t *w)
{
    const int nearly = w[HR_FRAMING_OK_THRESHOLD] - 1;
    w[HR_FLAGS_SEEN] = (w[HR_FLAGS_SEEN] < nearly)  ?  0  :  nearly;
}

// rx_flag_or_abort()
HDLC_HD void hdlc_rx_flag_or_abort(int32_t *w, HdlcBuf &buf, HdlcRxSink &out)
{
    const int thr = w[HR_FRAMING_OK_THRESHOLD];
    if ((uint32_t) w[HR_RAW_BIT_STREAM] & 0x0100u)
    {
        w[HR_RX_ABORTS]++;
        out.status(kSigAbort);
        hdlc_rx_back_off(w);
        hdlc_rx_octet_count(w, out, true);
    }
    else
    {
        w[HR_OCTET_COUNTING_MODE] = 0;
        if (w[HR_FLAGS_SEEN] >= thr)
        {
            const int len = w[HR_LEN];
            const int crc_bytes = w[HR_CRC_BYTES];
            if (len)
            {
                if (w[HR_NUM_BITS] == 7  &&  len >= crc_bytes  &&  len <= w[HR_MAX_FRAME_LEN])
                {
                    if (hdlc_rx_crc_good(w, buf))
                    {
                        w[HR_RX_FRAMES]++;
                        w[HR_RX_BYTES] += len - crc_bytes;
                        out.frame(buf, len - crc_bytes, true);
                    }
                    else
                    {
                        w[HR_RX_CRC_ERRORS]++;
                        if (w[HR_REPORT_BAD_FRAMES])
                            out.frame(buf, len - crc_bytes, false);
                    }
                }
                else
                {
                    if (w[HR_REPORT_BAD_FRAMES])
                        out.frame(buf, (len >= crc_bytes)  ?  (len - crc_bytes)  :  0, false);
                    w[HR_RX_LENGTH_ERRORS]++;
                }
            }
        }
        else
        {
            // flags of a preamble come back to back, except that the one which completes it may follow an abort unaligned
            if (w[HR_FLAGS_SEEN] != thr - 1  &&  w[HR_NUM_BITS] != 7)
                hdlc_rx_back_off(w);
            if (++w[HR_FLAGS_SEEN] >= thr  &&  !w[HR_FRAMING_OK_ANNOUNCED])
            {
                out.status(kSigFramingOk);
                w[HR_FRAMING_OK_ANNOUNCED] = 1;
            }
        }
    }
    w[HR_LEN] = 0;
    w[HR_NUM_BITS] = 0;
}

// hdlc_rx_put_bit_core(): the newest bit is bit 8 of raw_bit_stream
HDLC_HD void hdlc_rx_bit_core(int32_t *w, HdlcBuf &buf, HdlcRxSink &out)
{
    const uint32_t raw = (uint32_t) w[HR_RAW_BIT_STREAM];
    if ((raw & 0x3E00u) == 0x3E00u)
    {
        // five ones before this bit: a stuffed zero goes, six ones and a zero or a one are a flag or an abort
        if ((raw & 0x4100u) == 0)
            return;
        if ((raw & 0xFE00u) == 0x7E00u)
        {
            hdlc_rx_flag_or_abort(w, buf, out);
            return;
        }
    }
    w[HR_NUM_BITS]++;
    if (w[HR_FLAGS_SEEN] < w[HR_FRAMING_OK_THRESHOLD])
    {
        if ((w[HR_NUM_BITS] & 7) == 0)
            hdlc_rx_octet_count(w, out, false);
        return;
    }
    w[HR_BYTE_IN_PROGRESS] = (int32_t) ((((uint32_t) w[HR_BYTE_IN_PROGRESS]) | (raw & 0x100u)) >> 1);
    if (w[HR_NUM_BITS] == 8)
    {
        if (w[HR_LEN] < w[HR_MAX_FRAME_LEN])
        {
            buf.put(w[HR_LEN], w[HR_BYTE_IN_PROGRESS] & 0xFF);
            w[HR_LEN]++;
        }
        else
        {
            // too long: the frame is given up until the next flag
            w[HR_LEN] = kHdlcBuf + 1;
            w[HR_FLAGS_SEEN] = w[HR_FRAMING_OK_THRESHOLD] - 1;
            hdlc_rx_octet_count(w, out, true);
        }
        w[HR_NUM_BITS] = 0;
    }
}

// rx_special_condition()
HDLC_HD void hdlc_rx_special(int32_t *w, HdlcRxSink &out, int status)
{
    switch (status)
    {
    case kSigCarrierUp:
    case kSigTrainingSucceeded:
        w[HR_RAW_BIT_STREAM] = 0;
        w[HR_LEN] = 0;
        w[HR_NUM_BITS] = 0;
        w[HR_FLAGS_SEEN] = 0;
        w[HR_FRAMING_OK_ANNOUNCED] = 0;
        out.status(status);
        break;
    case kSigTrainingInProgress:
    case kSigTrainingFailed:
    case kSigCarrierDown:
    case kSigEndOfData:
        out.status(status);
        break;
    default:
        break;
    }
}

// hdlc_rx_put_bit()
HDLC_HD void hdlc_rx_event(int32_t *w, HdlcBuf &buf, HdlcRxSink &out, int ev)
{
    if (ev < 0)
    {
        hdlc_rx_special(w, out, ev);
        return;
    }
    w[HR_RAW_BIT_STREAM] = (int32_t) ((((uint32_t) w[HR_RAW_BIT_STREAM]) << 1) | (((uint32_t) ev << 8) & 0x100u));
    hdlc_rx_bit_core(w, buf, out);
}

// hdlc_rx_put_byte() of an octet: it is ORed into the low eight bits, then shifted up past bit 8 one bit at a time
HDLC_HD void hdlc_rx_octet(int32_t *w, HdlcBuf &buf, HdlcRxSink &out, int octet)
{
    w[HR_RAW_BIT_STREAM] = (int32_t) (((uint32_t) w[HR_RAW_BIT_STREAM]) | (uint32_t) octet);
    for (int i = 0;  i < 8;  i++)
    {
        w[HR_RAW_BIT_STREAM] = (int32_t) (((uint32_t) w[HR_RAW_BIT_STREAM]) << 1);
        hdlc_rx_bit_core(w, buf, out);
    }
}

// hdlc_rx_init() / hdlc_rx_restart()
HDLC_HD void hdlc_rx_words_init(int32_t *w, int crc32, int report_bad_frames, int framing_ok_threshold)
{
    for (int i = 0;  i < kHdlcRxWords;  i++)
        w[i] = 0;
    w[HR_CRC_BYTES] = crc32  ?  4  :  2;
    w[HR_REPORT_BAD_FRAMES] = report_bad_frames  ?  1  :  0;
    w[HR_FRAMING_OK_THRESHOLD] = (framing_ok_threshold < 1)  ?  1  :  framing_ok_threshold;
    w[HR_MAX_FRAME_LEN] = kHdlcBuf;
}

HDLC_HD void hdlc_rx_words_restart(int32_t *w)
{
    w[HR_FRAMING_OK_ANNOUNCED] = 0;
    w[HR_FLAGS_SEEN] = 0;
    w[HR_RAW_BIT_STREAM] = 0;
    w[HR_BYTE_IN_PROGRESS] = 0;
    w[HR_NUM_BITS] = 0;
    w[HR_OCTET_COUNTING_MODE] = 0;
    w[HR_OCTET_COUNT] = 0;
    w[HR_LEN] = 0;
}

// The most one call of `events` entries can hand to the handlers of a channel, whatever its state at entry.
//  Records.  An entry below zero is at most one status.  A bit ends in at most one handler call -- a frame, framing OK, an
//  octet report, an abort -- except an abort with octet counting on, which is two (the abort and the report).  An abort needs
//  a zero and seven ones behind it, so the aborts of a call are at least eight bits apart, and the first can come with the
//  first bit, on ones carried in: events + events/8 + 1.  (The run of 0x7F at report interval 1 has 2 records every 8 bits;
//  bad one-octet frames 16 bits apart, and octet reports at interval 1, one per 8 bits, are below that.)
//  Octets.  The first flag of a call can deliver what was carried in: len is at most 405 and at least 2 CRC octets come off,
//  403.  Every octet delivered after that was stored by this call, eight bits or more each: 403 + events/8, to a word.
HDLC_HD void hdlc_rx_capacity(long long events, long long *rec_cap, long long *byte_cap)
{
    *rec_cap = events + events/8 + 1;
    *byte_cap = (kHdlcBuf + 1 - 2 + events/8 + 3) & ~3LL;
}

// ---- sender ----------------------------------------------------------------------------------------------------------

// The command queue of one channel: `depth` slots, a header word and 404 bytes each.
struct HdlcTxQueue
{
    int32_t *hdr;           // [depth]
    const uint32_t *data;   // [depth][101] words
    int depth;
    int underflows;         // handler calls that found it empty
    int calls = 0;          // all handler calls (each is one SEND_STEP_COMPLETE under the FAX transmit front end)
};

// hdlc_tx_frame(s, slot, len), then hdlc_tx_corrupt_frame(s) where asked for
HDLC_HD void hdlc_tx_load_frame(int32_t *w, HdlcBuf &buf, const uint32_t *src, int len, bool corrupt)
{
    if (len <= 0  ||  len > w[HT_MAX_FRAME_LEN]  ||  w[HT_LEN])
        return;
    uint32_t crc = (uint32_t) w[HT_CRC];
    if (w[HT_CRC_BYTES] == 2)
        crc &= 0xFFFFu;
    for (int i = 0;  i < len;  i++)
    {
        const int octet = (int) ((src[i >> 2] >> (8*(i & 3))) & 0xFFu);
        buf.put(i, octet);
        crc = hdlc_crc_octet(crc, octet, w[HT_CRC_BYTES]);
    }
    w[HT_LEN] = len;
    w[HT_TX_END] = 0;
    if (corrupt)
    {
        // (0xFFFF whichever the CRC, as the reference has it; the four octets after the frame are the CRC of the one before)
        crc ^= 0xFFFFu;
        for (int i = 0;  i < 4;  i++)
            buf.put(kHdlcMaxFrame + i, buf.get(kHdlcMaxFrame + i) ^ 0xFF);
    }
    w[HT_CRC] = (int32_t) crc;
}

// hdlc_tx_flags(): not inside a frame
HDLC_HD void hdlc_tx_flags_now(int32_t *w, int len)
{
    if (w[HT_POS] == 0)
    {
        w[HT_FLAG_OCTETS] = (len < 0)  ?  (w[HT_FLAG_OCTETS] - len)  :  len;
        w[HT_REPORT_FLAG_UNDERFLOW] = 1;
        w[HT_TX_END] = 0;
    }
}

// One command off the queue, as the reference's call of that name would act on the state now.  False: nothing queued.
HDLC_HD bool hdlc_tx_take(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q)
{
    if (w[HT_Q_COUNT] <= 0)
        return false;
    const int slot = w[HT_Q_HEAD];
    const int32_t h = q.hdr[slot];
    const int arg = h >> 8;
    w[HT_Q_HEAD] = (slot + 1 == q.depth)  ?  0  :  (slot + 1);
    w[HT_Q_COUNT]--;
    switch (h & 7)
    {
    case kHdlcCmdFrame:
        hdlc_tx_load_frame(w, buf, q.data + (size_t) slot*kHdlcBufWords, arg, (h & kHdlcCmdCorrupt) != 0);
        break;
    case kHdlcCmdFlags:
        hdlc_tx_flags_now(w, arg);
        break;
    case kHdlcCmdAbort:
        w[HT_FLAG_OCTETS]++;
        w[HT_ABORT_OCTETS]++;
        break;
    case kHdlcCmdEnd:
        w[HT_TX_END] = 1;
        break;
    }
    return true;
}

// where the reference calls its underflow handler
HDLC_HD void hdlc_tx_underflow(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q)
{
    q.calls++;
    if (!hdlc_tx_take(w, buf, q))
        q.underflows++;
}

// between calls, an idle sender is offered the queue: commands until a frame is in or nothing is left
HDLC_HD void hdlc_tx_offer(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q)
{
    while (w[HT_LEN] == 0  &&  hdlc_tx_take(w, buf, q))
        ;
}

// hdlc_tx_get_byte()
HDLC_HD int hdlc_tx_get_byte(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q)
{
    if (w[HT_FLAG_OCTETS] > 0)
    {
        // timed flags: a preamble, the gap between frames, an abort
        if (--w[HT_FLAG_OCTETS] <= 0  &&  w[HT_REPORT_FLAG_UNDERFLOW])
        {
            w[HT_REPORT_FLAG_UNDERFLOW] = 0;
            if (w[HT_LEN] == 0)
                hdlc_tx_underflow(w, buf, q);
        }
        if (w[HT_ABORT_OCTETS])
        {
            w[HT_ABORT_OCTETS] = 0;
            return 0x7F;
        }
        return w[HT_IDLE_OCTET];
    }
    if (w[HT_LEN])
    {
        uint32_t oip = (uint32_t) w[HT_OCTETS_IN_PROGRESS];
        int nb = w[HT_NUM_BITS];
        if (nb >= 8)
        {
            // stuffing has gathered a whole octet
            nb -= 8;
            w[HT_NUM_BITS] = nb;
            return (int) ((oip >> nb) & 0xFFu);
        }
        const int crc_bytes = w[HT_CRC_BYTES];
        if (w[HT_POS] >= w[HT_LEN])
        {
            if (w[HT_POS] == w[HT_LEN])
            {
                // the CRC goes behind the longest frame, and the position jumps there
                const uint32_t crc = ~(uint32_t) w[HT_CRC];
                w[HT_CRC] = (int32_t) crc;
                for (int i = 0;  i < crc_bytes;  i++)
                    buf.put(kHdlcMaxFrame + i, (int) ((crc >> (8*i)) & 0xFFu));
                w[HT_POS] = kHdlcMaxFrame;
            }
            else if (w[HT_POS] == kHdlcMaxFrame + crc_bytes)
            {
                // the bits left over, filled up with the start of a flag; idling goes on with the flag rotated to match,
                // and the next frame starts on the rest of one
                const int txbyte = (int) (((oip << (8 - nb)) | (0x7Eu >> nb)) & 0xFFu);
                w[HT_IDLE_OCTET] = (0x7E7E >> nb) & 0xFF;
                w[HT_OCTETS_IN_PROGRESS] = w[HT_IDLE_OCTET] >> (8 - nb);
                w[HT_FLAG_OCTETS] = w[HT_INTER_FRAME_FLAGS] - 1;
                w[HT_LEN] = 0;
                w[HT_POS] = 0;
                w[HT_CRC] = (crc_bytes == 2)  ?  0xFFFF  :  (int32_t) 0xFFFFFFFFu;
                w[HT_REPORT_FLAG_UNDERFLOW] = 0;
                hdlc_tx_underflow(w, buf, q);
                // at least one whole flag where no new frame came
                if (w[HT_LEN] == 0  &&  w[HT_FLAG_OCTETS] < 2)
                    w[HT_FLAG_OCTETS] = 2;
                return txbyte;
            }
        }
        int octet = buf.get(w[HT_POS]);
        w[HT_POS]++;
        for (int i = 0;  i < 8;  i++)
        {
            oip = (oip << 1) | (uint32_t) (octet & 1);
            octet >>= 1;
            if ((oip & 0x1Fu) == 0x1Fu)
            {
                oip <<= 1;
                nb++;
            }
        }
        w[HT_OCTETS_IN_PROGRESS] = (int32_t) oip;
        w[HT_NUM_BITS] = nb;
        return (int) ((oip >> nb) & 0xFFu);
    }
    if (w[HT_TX_END])
    {
        w[HT_TX_END] = 0;
        return kSigEndOfData;
    }
    return w[HT_IDLE_OCTET];
}

// hdlc_tx_get_bit()
HDLC_HD int hdlc_tx_get_bit(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q)
{
    if (w[HT_BITS] == 0)
    {
        if ((w[HT_BYTE] = hdlc_tx_get_byte(w, buf, q)) < 0)
            return w[HT_BYTE];
        w[HT_BITS] = 8;
    }
    w[HT_BITS]--;
    return (w[HT_BYTE] >> w[HT_BITS]) & 1;
}

// One call on one channel: up to `want` bits, LSB first into bits[]; the number produced.  *ended: get_byte answered
// SIG_STATUS_END_OF_DATA, and the call stopped there.
HDLC_HD int hdlc_tx_run(int32_t *w, HdlcBuf &buf, HdlcTxQueue &q, uint8_t *bits, int want, int *ended)
{
    hdlc_tx_offer(w, buf, q);
    int acc = 0;
    int n = 0;
    *ended = 0;
    for (  ;  n < want;  n++)
    {
        const int bit = hdlc_tx_get_bit(w, buf, q);
        if (bit < 0)
        {
            *ended = 1;
            break;
        }
        acc |= bit << (n & 7);
        if ((n & 7) == 7)
        {
            bits[n >> 3] = (uint8_t) acc;
            acc = 0;
        }
    }
    if (n & 7)
        bits[n >> 3] = (uint8_t) acc;
    return n;
}

// hdlc_tx_init() / hdlc_tx_restart()
HDLC_HD void hdlc_tx_words_restart(int32_t *w)
{
    w[HT_OCTETS_IN_PROGRESS] = 0;
    w[HT_NUM_BITS] = 0;
    w[HT_IDLE_OCTET] = 0x7E;
    w[HT_FLAG_OCTETS] = 0;
    w[HT_ABORT_OCTETS] = 0;
    w[HT_REPORT_FLAG_UNDERFLOW] = 0;
    w[HT_LEN] = 0;
    w[HT_POS] = 0;
    w[HT_CRC] = (w[HT_CRC_BYTES] == 2)  ?  0xFFFF  :  (int32_t) 0xFFFFFFFFu;
    w[HT_BYTE] = 0;
    w[HT_BITS] = 0;
    w[HT_TX_END] = 0;
}

HDLC_HD void hdlc_tx_words_init(int32_t *w, int crc32, int inter_frame_flags)
{
    for (int i = 0;  i < kHdlcTxWords;  i++)
        w[i] = 0;
    w[HT_CRC_BYTES] = crc32  ?  4  :  2;
    w[HT_INTER_FRAME_FLAGS] = (inter_frame_flags < 1)  ?  1  :  inter_frame_flags;
    w[HT_MAX_FRAME_LEN] = kHdlcMaxFrame;
    hdlc_tx_words_restart(w);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
// (a unit that wants the step functions alone, for a kernel of its own, defines SPG_HDLC_STEP_FUNCTIONS_ONLY: the sender's
// kernels are not templates and belong to one unit)

#if defined(__HIPCC__)  &&  !defined(SPG_HDLC_STEP_FUNCTIONS_ONLY)

struct HdlcRxLaunch
{
    int32_t *st;
    uint32_t *buf;
    int n_ch;
    const void *events;         // [n_ch][cap] of E, or octets [n_ch][cap]
    long long cap;              // entries per row
    const int32_t *counts;      // [n_ch]; NULL: `all` entries of every row
    int all;
    int vec;                    // rows start on 16 bytes and are a multiple of 16 bytes long
    int32_t *recs;              // [n_ch][rec_cap]
    uint8_t *bytes;             // [n_ch][byte_cap]
    int32_t *rec_counts;        // [n_ch]
    int32_t *byte_counts;       // [n_ch]
    int rec_cap;
    int byte_cap;
};

// E: int8_t or int16_t events; uint8_t: octets, most significant bit first
template <typename E>
__global__ __launch_bounds__(64) void hdlc_rx_kernel(HdlcRxLaunch L)
{
    const int ch = blockIdx.x*64 + threadIdx.x;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    HdlcRxSink out;
    out.recs = L.recs + (size_t) ch*L.rec_cap;
    out.bytes = L.bytes + (size_t) ch*L.byte_cap;
    out.rec_cap = L.rec_cap;
    out.byte_cap = L.byte_cap;
    out.n_recs = 0;
    out.n_bytes = 0;
    int count = L.counts  ?  L.counts[ch]  :  L.all;
    count = (count < 0)  ?  0  :  ((count > L.cap)  ?  (int) L.cap  :  count);
    if (count > 0)
    {
        int32_t w[kHdlcRxWords];
        for (int i = 0;  i < kHdlcRxWords;  i++)
            w[i] = L.st[(size_t) i*n + ch];
        HdlcBuf buf;
        buf.open(L.buf + ch, n);
        const E *row = (const E *) L.events + (size_t) ch*L.cap;
        constexpr int kPer = 16/(int) sizeof(E);
        int i = 0;
        if (L.vec)
        {
            for (  ;  i + kPer <= count;  i += kPer)
            {
                const uint4 v = *reinterpret_cast<const uint4 *>(row + i);
                const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0;  k < kPer;  k++)
                {
                    const uint32_t bits = q[k*(int) sizeof(E)/4] >> (8*((k*(int) sizeof(E)) & 3));
                    if (sizeof(E) == 2)
                        hdlc_rx_event(w, buf, out, (int) (int16_t) (bits & 0xFFFFu));
                    else if (E(-1) < E(0))
                        hdlc_rx_event(w, buf, out, (int) (int8_t) (bits & 0xFFu));
                    else
                        hdlc_rx_octet(w, buf, out, (int) (bits & 0xFFu));
                }
            }
        }
        for (  ;  i < count;  i++)
        {
            if (E(-1) < E(0))
                hdlc_rx_event(w, buf, out, (int) row[i]);
            else
                hdlc_rx_octet(w, buf, out, (int) row[i]);
        }
        buf.close();
        for (int k = 0;  k < kHdlcRxWords;  k++)
            L.st[(size_t) k*n + ch] = w[k];
    }
    L.rec_counts[ch] = out.n_recs;
    L.byte_counts[ch] = out.n_bytes;
}

struct HdlcTxLaunch
{
    int32_t *st;
    uint32_t *buf;
    int n_ch;
    int32_t *q_hdr;             // [n_ch][depth]
    uint32_t *q_data;           // [n_ch][depth][101]
    int depth;
    uint8_t *bits;              // [n_ch][stride]
    long long stride;
    const int32_t *want;        // [n_ch]; NULL: want_all
    int want_all;
    int32_t *lens;              // [n_ch]
    int32_t *ended;             // [n_ch]
    int32_t *underflows;        // [n_ch]
};

__global__ __launch_bounds__(64) void hdlc_tx_kernel(HdlcTxLaunch L)
{
    const int ch = blockIdx.x*64 + threadIdx.x;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int want = L.want  ?  L.want[ch]  :  L.want_all;
    want = (want < 0)  ?  0  :  ((want > L.stride*8)  ?  (int) (L.stride*8)  :  want);
    int got = 0;
    int ended = 0;
    int underflows = 0;
    // a channel asked for nothing sits the call out: its state and its queue as they were
    if (want > 0)
    {
        int32_t w[kHdlcTxWords];
        for (int i = 0;  i < kHdlcTxWords;  i++)
            w[i] = L.st[(size_t) i*n + ch];
        HdlcBuf buf;
        buf.open(L.buf + ch, n);
        HdlcTxQueue q;
        q.hdr = L.q_hdr + (size_t) ch*L.depth;
        q.data = L.q_data + (size_t) ch*L.depth*kHdlcBufWords;
        q.depth = L.depth;
        q.underflows = 0;
        got = hdlc_tx_run(w, buf, q, L.bits + (size_t) ch*L.stride, want, &ended);
        underflows = q.underflows;
        buf.close();
        for (int i = 0;  i < kHdlcTxWords;  i++)
            L.st[(size_t) i*n + ch] = w[i];
    }
    L.lens[ch] = got;
    L.ended[ch] = ended;
    L.underflows[ch] = underflows;
}

// Commands for channels [lo, hi): kind as above; FRAME takes frames[(ch - lo)*fstride ..], lens[ch - lo] octets (below
// zero: nothing for this channel) and flags[ch - lo] & 1 = corrupt; FLAGS takes lens[ch - lo] as its count.
// results[ch - lo]: 0, or -1 where the queue is full or the reference would refuse the length.
__global__ void hdlc_tx_enqueue_kernel(int32_t *st, int n_ch, int32_t *q_hdr, uint32_t *q_data, int depth, int lo, int hi, int kind,
                                       const uint8_t *frames, int fstride, const int32_t *lens, const int32_t *flags, int32_t *results)
{
    const int ch = lo + blockIdx.x*blockDim.x + threadIdx.x;
    if (ch >= hi)
        return;
    const size_t n = (size_t) n_ch;
    const int len = lens  ?  lens[ch - lo]  :  0;
    if (kind == kHdlcCmdFrame  &&  len < 0)
    {
        results[ch - lo] = 0;
        return;
    }
    const int count = st[(size_t) HT_Q_COUNT*n + ch];
    if (count >= depth  ||  (kind == kHdlcCmdFrame  &&  (len > st[(size_t) HT_MAX_FRAME_LEN*n + ch]  ||  len > fstride)))
    {
        results[ch - lo] = -1;
        return;
    }
    int slot = st[(size_t) HT_Q_HEAD*n + ch] + count;
    slot -= (slot >= depth)  ?  depth  :  0;
    int32_t h = kind;
    if (kind == kHdlcCmdFrame)
    {
        // hdlc_tx_frame(s, NULL, 0) is the end of the data
        if (len == 0)
            h = kHdlcCmdEnd;
        else
        {
            const uint8_t *src = frames + (size_t) (ch - lo)*fstride;
            uint32_t *dst = q_data + ((size_t) ch*depth + slot)*kHdlcBufWords;
            for (int i = 0;  i < len;  i += 4)
            {
                uint32_t v = 0;
                for (int k = 0;  k < 4  &&  i + k < len;  k++)
                    v |= (uint32_t) src[i + k] << (8*k);
                dst[i >> 2] = v;
            }
            h = kHdlcCmdFrame | ((flags  &&  (flags[ch - lo] & 1))  ?  kHdlcCmdCorrupt  :  0) | (len << 8);
        }
    }
    else if (kind == kHdlcCmdFlags)
        h = kHdlcCmdFlags | (int32_t) ((uint32_t) len << 8);
    q_hdr[(size_t) ch*depth + slot] = h;
    st[(size_t) HT_Q_COUNT*n + ch] = count + 1;
    results[ch - lo] = 0;
}

#endif  // __HIPCC__

}   // namespace spg
