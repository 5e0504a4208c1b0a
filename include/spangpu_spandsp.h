/*
 * spangpu_spandsp.h -- the spandsp-named, per-channel C entry points of libspangpu.so.
 *
 * Source-compatible with the reference's public tone-detector API: same names, argument
 * order, return values and callback types, so an existing caller (FreeSWITCH mod_spandsp,
 * adsi.c, v18.c ...) re-links unchanged.  State objects are opaque (the reference exposes
 * them only through its private headers).  Behind each object is one channel slot of a
 * GPU bank (include/spangpu.h):
 *
 *   - xxx_rx_init(NULL, ...) makes a PRIVATE one-channel bank: xxx_rx() then runs the frame
 *     on the GPU and replays callbacks before it returns -- same observable behaviour, per
 *     call, as the reference (this is the plumbing configuration);
 *   - spangpu_group_create() + spangpu_xxx_rx_attach() put N objects on ONE bank: each
 *     xxx_rx() stages its frame (from any thread; one submitter per object), and when every
 *     attached channel has staged -- or when the tick's owner calls spangpu_group_flush() at
 *     its deadline, with whoever staged: a silent or late channel stalls nobody and is itself
 *     untouched -- a single kernel launch advances the channels that take part and their
 *     callbacks are replayed in channel order, each channel's events in sample order.  This
 *     is the production configuration (thousands of channels / launch).
 *
 * Reference declarations being replaced (relative to the reference tree):
 *   dtmf_rx_init/_release/_free            src/spandsp/dtmf.h:216-228     src/dtmf.c:447-519
 *   dtmf_rx                                src/spandsp/dtmf.h:177         src/dtmf.c:132-361
 *   dtmf_rx_fillin/_status/_get            src/spandsp/dtmf.h:185-201     src/dtmf.c:363-408
 *   dtmf_rx_parms/_set_realtime_callback   src/spandsp/dtmf.h:153-170     src/dtmf.c:410-445
 *   bell_mf_rx_init/_rx/_get/_release/_free  src/spandsp/bell_r2_mf.h:199-228  src/bell_r2_mf.c:507-748
 *   r2_mf_rx_init/_rx/_get/_release/_free  src/spandsp/bell_r2_mf.h:236-266  src/bell_r2_mf.c:750-951
 *   super_tone_rx_* (descriptor + detector)  src/spandsp/super_tone_rx.h:76-164  src/super_tone_rx.c:81-568
 *   goertzel_*  / make_goertzel_descriptor src/spandsp/tone_detect.h:86-124  src/tone_detect.c:60-205
 *   echo_can_init/_release/_free/_flush/_adaption_mode/_update/_hpf_tx
 *                                          src/spandsp/echo.h:145-185     src/echo.c:254-380,421-669
 *   v29_rx_init/_restart/_release/_free/_set_put_bit/_set_modem_status_handler/_set_qam_report_handler/_rx/_fillin/_equalizer_state/
 *     _carrier_frequency/_symbol_timing_correction/_signal_power/_set_signal_cutoff
 *                                          src/spandsp/v29rx.h:151-244    src/v29rx.c:139-196,867-1148
 *   v27ter_rx_* (same set)                 src/spandsp/v27ter_rx.h:71-165 src/v27ter_rx.c:136-170,863-1210
 *   v17_rx_* (same set)                    src/spandsp/v17rx.h:236-333    src/v17rx.c:165-212,1212-1541
 * Callback types: digits_rx_callback_t (dtmf.h:76), span_tone_report_func_t and
 * tone_segment_func_t (super_tone_rx.h:56-58), span_put_bit_func_t and span_modem_status_func_t
 * (async.h:123,131), qam_report_handler_t (v29rx.h:130).  xxx_rx_get_logging_state() hands out a
 * logging_state_t with the layout spandsp's span_log_*() functions work on (private/logging.h:32-42).
 *   filter_create/_delete/_step, cfilter_create/_delete/_step
 *                                          src/spandsp/complex_filters.h:62-68   src/complex_filters.c:39-118
 *   echo_can_snapshot                      src/spandsp/echo.h:185          src/echo.c:376-379
 */
#if !defined(SPANGPU_SPANDSP_H)
#define SPANGPU_SPANDSP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "spangpu.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* The logging descriptor the reference's receivers carry (src/spandsp/private/logging.h:32-42): same fields in the same
   order, so that a caller that links spandsp's logging.c can hand the pointer xxx_rx_get_logging_state() returns to
   span_log_set_level() / span_log_set_tag() as it does today.  The engine itself never writes log text. */
typedef void (*message_handler_func_t)(void *user_data, int level, const char *text);
typedef struct logging_state_s
{
    int level;
    int samples_per_second;
    int64_t elapsed_samples;
    const char *tag;
    const char *protocol;
    message_handler_func_t span_message;
    void *user_data;
} logging_state_t;

/* What every lone object -- one that owns a private one-channel bank -- keeps beside its bank (csrc/shim_object.h): the row a
   launch's piece comes back in before the caller's buffer gets its count of it, and who owns the object's storage. */
typedef struct
{
    void *row;
    size_t row_cap;             /* bytes */
    int caller_storage;
} spangpu_object_t;

typedef void (*digits_rx_callback_t)(void *user_data, const char *digits, int len);
typedef void (*span_tone_report_func_t)(void *user_data, int code, int level, int delay);
typedef void (*tone_segment_func_t)(void *data, int f1, int f2, int duration);

#define MAX_DTMF_DIGITS         128
#define MAX_BELL_MF_DIGITS      128

typedef struct dtmf_rx_state_s dtmf_rx_state_t;
typedef struct bell_mf_rx_state_s bell_mf_rx_state_t;
typedef struct r2_mf_rx_state_s r2_mf_rx_state_t;
typedef struct super_tone_rx_descriptor_s super_tone_rx_descriptor_t;
typedef struct super_tone_rx_state_s super_tone_rx_state_t;
typedef struct goertzel_state_s goertzel_state_t;
typedef struct
{
    float fac;
    int samples;
} goertzel_descriptor_t;

/* ---- modem receivers ------------------------------------------------------------------ */
typedef void (*span_put_bit_func_t)(void *user_data, int bit);
typedef void (*span_modem_status_func_t)(void *user_data, int status);

typedef struct
{
    float re;
    float im;
} complexf_t;

/* spandsp/v29rx.h:130: the per-baud constellation tap (constel and target are NULL for V.27ter's timing hop report) */
typedef void (*qam_report_handler_t)(void *user_data, const complexf_t *constel, const complexf_t *target, int symbol);

/* spandsp/async.h:66-103: the status codes a receiver passes through put_bit / the status handler */
enum
{
    SIG_STATUS_CARRIER_DOWN = -1,
    SIG_STATUS_CARRIER_UP = -2,
    SIG_STATUS_TRAINING_IN_PROGRESS = -3,
    SIG_STATUS_TRAINING_SUCCEEDED = -4,
    SIG_STATUS_TRAINING_FAILED = -5,
    SIG_STATUS_END_OF_DATA = -7,
    SIG_STATUS_SHUTDOWN_COMPLETE = -10,
    SIG_STATUS_LINK_IDLE = -17
};

typedef struct v29_rx_state_s v29_rx_state_t;
typedef struct v27ter_rx_state_s v27ter_rx_state_t;
typedef struct v17_rx_state_s v17_rx_state_t;
typedef struct spangpu_modem_group_s spangpu_modem_group_t;

/* N receivers of one kind (SPANGPU_V29 / _V27TER / _V17) and bit rate on one bank; as for the tone groups, each
   xxx_rx() stages its frame and the last attached channel of the tick (or spangpu_modem_group_flush()) launches. */
SPANGPU_API spangpu_modem_group_t *spangpu_modem_group_create(int device, int kind, int n_channels, int bit_rate, int max_samples);
SPANGPU_API int spangpu_modem_group_destroy(spangpu_modem_group_t *g);
SPANGPU_API int spangpu_modem_group_flush(spangpu_modem_group_t *g);
SPANGPU_API spangpu_modem_t *spangpu_modem_group_bank(spangpu_modem_group_t *g);

SPANGPU_API v29_rx_state_t *v29_rx_init(v29_rx_state_t *s, int bit_rate, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API v29_rx_state_t *spangpu_v29_rx_attach(spangpu_modem_group_t *g, int channel, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API int v29_rx(v29_rx_state_t *s, const int16_t amp[], int len);
SPANGPU_API int v29_rx_fillin(v29_rx_state_t *s, int len);
SPANGPU_API int v29_rx_release(v29_rx_state_t *s);
SPANGPU_API int v29_rx_free(v29_rx_state_t *s);
SPANGPU_API void v29_rx_set_put_bit(v29_rx_state_t *s, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API void v29_rx_set_modem_status_handler(v29_rx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API void v29_rx_set_qam_report_handler(v29_rx_state_t *s, qam_report_handler_t handler, void *user_data);
SPANGPU_API int v29_rx_equalizer_state(v29_rx_state_t *s, complexf_t **coeffs);
SPANGPU_API float v29_rx_carrier_frequency(v29_rx_state_t *s);
SPANGPU_API float v29_rx_symbol_timing_correction(v29_rx_state_t *s);
SPANGPU_API float v29_rx_signal_power(v29_rx_state_t *s);
SPANGPU_API logging_state_t *v29_rx_get_logging_state(v29_rx_state_t *s);          /* src/spandsp/v29rx.h:177 */
SPANGPU_API void v29_rx_set_signal_cutoff(v29_rx_state_t *s, float cutoff);

SPANGPU_API v27ter_rx_state_t *v27ter_rx_init(v27ter_rx_state_t *s, int bit_rate, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API v27ter_rx_state_t *spangpu_v27ter_rx_attach(spangpu_modem_group_t *g, int channel, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API int v27ter_rx(v27ter_rx_state_t *s, const int16_t amp[], int len);
SPANGPU_API int v27ter_rx_fillin(v27ter_rx_state_t *s, int len);
SPANGPU_API int v27ter_rx_release(v27ter_rx_state_t *s);
SPANGPU_API int v27ter_rx_free(v27ter_rx_state_t *s);
SPANGPU_API void v27ter_rx_set_put_bit(v27ter_rx_state_t *s, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API void v27ter_rx_set_modem_status_handler(v27ter_rx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API void v27ter_rx_set_qam_report_handler(v27ter_rx_state_t *s, qam_report_handler_t handler, void *user_data);
SPANGPU_API int v27ter_rx_equalizer_state(v27ter_rx_state_t *s, complexf_t **coeffs);
SPANGPU_API float v27ter_rx_carrier_frequency(v27ter_rx_state_t *s);
SPANGPU_API float v27ter_rx_symbol_timing_correction(v27ter_rx_state_t *s);
SPANGPU_API float v27ter_rx_signal_power(v27ter_rx_state_t *s);
SPANGPU_API logging_state_t *v27ter_rx_get_logging_state(v27ter_rx_state_t *s);
SPANGPU_API void v27ter_rx_set_signal_cutoff(v27ter_rx_state_t *s, float cutoff);

SPANGPU_API v17_rx_state_t *v17_rx_init(v17_rx_state_t *s, int bit_rate, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API v17_rx_state_t *spangpu_v17_rx_attach(spangpu_modem_group_t *g, int channel, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API int v17_rx(v17_rx_state_t *s, const int16_t amp[], int len);
SPANGPU_API int v17_rx_fillin(v17_rx_state_t *s, int len);
SPANGPU_API int v17_rx_release(v17_rx_state_t *s);
SPANGPU_API int v17_rx_free(v17_rx_state_t *s);
SPANGPU_API void v17_rx_set_put_bit(v17_rx_state_t *s, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API void v17_rx_set_modem_status_handler(v17_rx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API void v17_rx_set_qam_report_handler(v17_rx_state_t *s, qam_report_handler_t handler, void *user_data);
SPANGPU_API int v17_rx_equalizer_state(v17_rx_state_t *s, complexf_t **coeffs);
SPANGPU_API float v17_rx_carrier_frequency(v17_rx_state_t *s);
SPANGPU_API float v17_rx_symbol_timing_correction(v17_rx_state_t *s);
SPANGPU_API float v17_rx_signal_power(v17_rx_state_t *s);
SPANGPU_API logging_state_t *v17_rx_get_logging_state(v17_rx_state_t *s);
SPANGPU_API void v17_rx_set_signal_cutoff(v17_rx_state_t *s, float cutoff);

SPANGPU_API int v29_rx_restart(v29_rx_state_t *s, int bit_rate, bool old_train);
SPANGPU_API int v27ter_rx_restart(v27ter_rx_state_t *s, int bit_rate, bool old_train);
SPANGPU_API int v17_rx_restart(v17_rx_state_t *s, int bit_rate, int short_train);

/* ---- echo canceller ---------------------------------------------------------------------- */
/* src/spandsp/echo.h:120-131 */
enum
{
    ECHO_CAN_USE_ADAPTION = 0x01,
    ECHO_CAN_USE_NLP = 0x02,
    ECHO_CAN_USE_CNG = 0x04,
    ECHO_CAN_USE_CLIP = 0x08,
    ECHO_CAN_USE_SUPPRESSOR = 0x10,
    ECHO_CAN_USE_TX_HPF = 0x20,
    ECHO_CAN_USE_RX_HPF = 0x40,
    ECHO_CAN_DISABLE = 0x80
};

typedef struct echo_can_state_s echo_can_state_t;

/* len (taps) must be a power of two from 32 to 1024.  An object made by echo_can_init() is a one-channel bank of its own:
   echo_can_update() is one kernel launch per sample and spangpu_echo_can_update_block() one launch per object -- source
   compatibility.  For throughput attach the objects to an echo group (spangpu_echo_can_attach(), below: N objects on one
   launch per tick), or hand the rows of N channels to spangpu_echo_update() / spangpu_echo_update_var(). */
SPANGPU_API echo_can_state_t *echo_can_init(int len, int adaption_mode);
SPANGPU_API int echo_can_release(echo_can_state_t *ec);
SPANGPU_API int echo_can_free(echo_can_state_t *ec);
SPANGPU_API void echo_can_flush(echo_can_state_t *ec);
/* echo_can_snapshot(): keep a copy of tap set 0 as it is now (src/echo.c:376-379; the reference keeps it in a private
   field).  spangpu_echo_can_snapshot_taps() hands the copy out: taps int16 values, returns the count. */
SPANGPU_API void echo_can_snapshot(echo_can_state_t *ec);
SPANGPU_API int spangpu_echo_can_snapshot_taps(echo_can_state_t *ec, int16_t *out, int max);
SPANGPU_API void echo_can_adaption_mode(echo_can_state_t *ec, int adaption_mode);
/* (a kernel launch per sample: build with -DSPANGPU_WARN_SLOW_CALLS to have the compiler point at every call site) */
#if defined(SPANGPU_WARN_SLOW_CALLS)
#define SPANGPU_SLOW_CALL(msg) __attribute__((deprecated(msg)))
#else
#define SPANGPU_SLOW_CALL(msg)
#endif
SPANGPU_API int16_t echo_can_update(echo_can_state_t *ec, int16_t tx, int16_t rx)
    SPANGPU_SLOW_CALL("one kernel launch per sample: use spangpu_echo_can_update_block() or spangpu_echo_update()");
SPANGPU_API int16_t echo_can_hpf_tx(echo_can_state_t *ec, int16_t tx)
    SPANGPU_SLOW_CALL("one kernel launch per sample: use spangpu_echo_can_update_block(..., use_hpf_tx = 1)");
SPANGPU_API int spangpu_echo_can_update_block(echo_can_state_t *ec, const int16_t tx[], const int16_t rx[], int16_t clean[],
                                              int16_t tx_out[], int n, int use_hpf_tx);
SPANGPU_API spangpu_echo_t *spangpu_echo_can_bank(echo_can_state_t *ec);

/* ---- echo canceller groups: N echo_can_state_t objects on one bank, one launch per tick -------------------------------
   spangpu_echo_can_attach() makes the object of one channel of the group: what echo_can_init(taps, adaption_mode) makes,
   also in a slot that another object has used before.  On an attached object
     spangpu_echo_can_update_block(ec, tx, rx, clean, tx_out, n, use_hpf_tx)
   copies tx / rx into the group's staging rows, REMEMBERS clean and tx_out, and returns SPANGPU_OK (n <= 0: 0, nothing is
   staged; n > max_samples: SPANGPU_ERR_BAD_ARG; a second frame before the tick ran: SPANGPU_ERR_STATE, the staged frame is
   kept).  The tick runs inside the call that completes the set -- every attached object has staged -- or in
   spangpu_echo_group_flush(), with the objects that have staged; the others sit it out, exactly as they were.  Frames of a
   tick may differ in length and in use_hpf_tx.  When the call that ran the tick returns, clean[] (and tx_out[]) of every
   object that took part are filled and its spangpu_echo_can_pending() is 0: THE CALLER KEEPS clean / tx_out VALID UNTIL
   THEN.  An object has one submitter; the objects of a group may be staged from different threads (one mutex per group,
   the tick runs on the thread that completes it).
   echo_can_flush(), echo_can_adaption_mode(), echo_can_snapshot(), spangpu_echo_can_snapshot_taps() and
   spangpu_echo_can_bank() (the group's bank) act on the object's channel alone and in call order: if the object has a frame
   pending, the tick runs first.  echo_can_update() / echo_can_hpf_tx() on an attached object stay correct -- pending work
   runs, then a launch over that one channel -- and stay slow.  echo_can_free() detaches: a pending frame is dropped, its
   buffers are not written, the slot may be attached again. */
typedef struct spangpu_echo_group_s spangpu_echo_group_t;
SPANGPU_API spangpu_echo_group_t *spangpu_echo_group_create(int device, int n_channels, int taps, int max_samples);
SPANGPU_API int spangpu_echo_group_destroy(spangpu_echo_group_t *g);
/* Run the tick with what is staged.  Returns the number of channels that took part, or a negative SPANGPU_ERR_*. */
SPANGPU_API int spangpu_echo_group_flush(spangpu_echo_group_t *g);
SPANGPU_API long long spangpu_echo_group_ticks(const spangpu_echo_group_t *g);      /* ticks run so far */
SPANGPU_API spangpu_echo_t *spangpu_echo_group_bank(spangpu_echo_group_t *g);
SPANGPU_API echo_can_state_t *spangpu_echo_can_attach(spangpu_echo_group_t *g, int channel, int adaption_mode);
SPANGPU_API int spangpu_echo_can_pending(echo_can_state_t *ec);                     /* 1 while a staged frame has not run */

/* ---- channel groups: N spandsp objects on one GPU bank ----------------------------- */
typedef struct spangpu_group_s spangpu_group_t;

/* kind: SPANGPU_DTMF / _BELL_MF / _R2_MF / _SUPER_TONE.  params may be NULL (defaults).
   max_samples bounds the samples one xxx_rx() call may carry (e.g. 160). */
SPANGPU_API spangpu_group_t *spangpu_group_create(int device, int kind, int n_channels, int max_samples,
                                                  const spangpu_tone_params_t *params);
SPANGPU_API int spangpu_group_destroy(spangpu_group_t *g);
/* Run the tick now: every attached channel must have staged a frame of the same length.
   Returns the number of channels processed, or a negative SPANGPU_ERR_*. */
SPANGPU_API int spangpu_group_flush(spangpu_group_t *g);
SPANGPU_API spangpu_bank_t *spangpu_group_bank(spangpu_group_t *g);

SPANGPU_API dtmf_rx_state_t *spangpu_dtmf_rx_attach(spangpu_group_t *g, int channel,
                                                    digits_rx_callback_t callback, void *user_data);
SPANGPU_API bell_mf_rx_state_t *spangpu_bell_mf_rx_attach(spangpu_group_t *g, int channel,
                                                          digits_rx_callback_t callback, void *user_data);
SPANGPU_API r2_mf_rx_state_t *spangpu_r2_mf_rx_attach(spangpu_group_t *g, int channel,
                                                      span_tone_report_func_t callback, void *user_data);
SPANGPU_API super_tone_rx_state_t *spangpu_super_tone_rx_attach(spangpu_group_t *g, int channel,
                                                                super_tone_rx_descriptor_t *desc,
                                                                span_tone_report_func_t callback, void *user_data);

/* Bank parameters (bin count and taps) for a super-tone group whose channels all use `desc`. */
SPANGPU_API int spangpu_super_tone_params(const super_tone_rx_descriptor_t *desc, spangpu_tone_params_t *params);
/* ... and its cadences, for spangpu_bank_cadence_events() (matched on the device; include/spangpu.h) */
SPANGPU_API int spangpu_super_tone_cadences(const super_tone_rx_descriptor_t *desc, spangpu_bank_t *bank, int want_segments);

/* ---- DTMF (src/spandsp/dtmf.h) -------------------------------------------------------- */
SPANGPU_API dtmf_rx_state_t *dtmf_rx_init(dtmf_rx_state_t *s, digits_rx_callback_t callback, void *user_data);
SPANGPU_API int dtmf_rx_release(dtmf_rx_state_t *s);
SPANGPU_API int dtmf_rx_free(dtmf_rx_state_t *s);
SPANGPU_API void dtmf_rx_set_realtime_callback(dtmf_rx_state_t *s, span_tone_report_func_t callback, void *user_data);
SPANGPU_API void dtmf_rx_parms(dtmf_rx_state_t *s, int filter_dialtone, float twist, float reverse_twist, float threshold);
SPANGPU_API int dtmf_rx(dtmf_rx_state_t *s, const int16_t amp[], int samples);
SPANGPU_API int dtmf_rx_fillin(dtmf_rx_state_t *s, int samples);
SPANGPU_API int dtmf_rx_status(dtmf_rx_state_t *s);
SPANGPU_API size_t dtmf_rx_get(dtmf_rx_state_t *s, char *digits, int max);
SPANGPU_API logging_state_t *dtmf_rx_get_logging_state(dtmf_rx_state_t *s);        /* src/spandsp/dtmf.h:206 */

/* ---- Bell MF / R2 MF (src/spandsp/bell_r2_mf.h) ------------------------------------------ */
SPANGPU_API bell_mf_rx_state_t *bell_mf_rx_init(bell_mf_rx_state_t *s, digits_rx_callback_t callback, void *user_data);
SPANGPU_API int bell_mf_rx_release(bell_mf_rx_state_t *s);
SPANGPU_API int bell_mf_rx_free(bell_mf_rx_state_t *s);
SPANGPU_API int bell_mf_rx(bell_mf_rx_state_t *s, const int16_t amp[], int samples);
SPANGPU_API size_t bell_mf_rx_get(bell_mf_rx_state_t *s, char *buf, int max);

SPANGPU_API r2_mf_rx_state_t *r2_mf_rx_init(r2_mf_rx_state_t *s, bool fwd, span_tone_report_func_t callback, void *user_data);
SPANGPU_API int r2_mf_rx_release(r2_mf_rx_state_t *s);
SPANGPU_API int r2_mf_rx_free(r2_mf_rx_state_t *s);
SPANGPU_API int r2_mf_rx(r2_mf_rx_state_t *s, const int16_t amp[], int samples);
SPANGPU_API int r2_mf_rx_get(r2_mf_rx_state_t *s);

/* ---- Super tone (src/spandsp/super_tone_rx.h) ----------------------------------------------- */
SPANGPU_API super_tone_rx_descriptor_t *super_tone_rx_make_descriptor(super_tone_rx_descriptor_t *desc);
SPANGPU_API int super_tone_rx_free_descriptor(super_tone_rx_descriptor_t *desc);
SPANGPU_API int super_tone_rx_add_tone(super_tone_rx_descriptor_t *desc);
SPANGPU_API int super_tone_rx_add_element(super_tone_rx_descriptor_t *desc, int tone, int f1, int f2, int min, int max);
SPANGPU_API super_tone_rx_state_t *super_tone_rx_init(super_tone_rx_state_t *s, super_tone_rx_descriptor_t *desc,
                                                      span_tone_report_func_t callback, void *user_data);
SPANGPU_API int super_tone_rx_release(super_tone_rx_state_t *s);
SPANGPU_API int super_tone_rx_free(super_tone_rx_state_t *s);
SPANGPU_API void super_tone_rx_tone_callback(super_tone_rx_state_t *s, span_tone_report_func_t callback, void *user_data);
SPANGPU_API void super_tone_rx_segment_callback(super_tone_rx_state_t *s, tone_segment_func_t callback);
SPANGPU_API int super_tone_rx(super_tone_rx_state_t *s, const int16_t amp[], int samples);
SPANGPU_API int super_tone_rx_fillin(super_tone_rx_state_t *s, int samples);

/* ---- Goertzel (src/spandsp/tone_detect.h) ------------------------------------------------------ */
SPANGPU_API void make_goertzel_descriptor(goertzel_descriptor_t *t, float freq, int samples);
SPANGPU_API goertzel_state_t *goertzel_init(goertzel_state_t *s, goertzel_descriptor_t *t);
SPANGPU_API int goertzel_release(goertzel_state_t *s);
SPANGPU_API int goertzel_free(goertzel_state_t *s);

/* ---- complex_filters.h: a filter instance around a caller-supplied step function (src/complex_filters.c:39-118).  The
   arithmetic of a filter is its fspec_t's fsf callback; these entry points only own the state it works on.  Host side only. */
typedef struct filter_s filter_t;
typedef float (*filter_step_func_t)(filter_t *fi, float x);
typedef struct
{
    int nz;
    int np;
    filter_step_func_t fsf;
} fspec_t;
struct filter_s
{
    fspec_t *fs;
    float sum;
    int ptr;                    /* only for moving average filters */
    float v[];
};
typedef struct
{
    filter_t *ref;
    filter_t *imf;
} cfilter_t;
SPANGPU_API filter_t *filter_create(fspec_t *fs);
SPANGPU_API void filter_delete(filter_t *fi);
SPANGPU_API float filter_step(filter_t *fi, float x);
SPANGPU_API cfilter_t *cfilter_create(fspec_t *fs);
SPANGPU_API void cfilter_delete(cfilter_t *cfi);
SPANGPU_API complexf_t cfilter_step(cfilter_t *cfi, const complexf_t *z);
/* The receivers' inner primitives under their spandsp names (vec_*, cvec_*, power_meter_*, godard_ted_*, periodogram*) are
 * NOT in libspangpu.so: libspandsp calls them from inside its own modules (fsk, v22bis, the modem receivers ...), and a process
 * that loads both libraries would have those internal calls bound here.  They live in libspangpu_prims.so, which a caller
 * links only when it wants them: include/spangpu_prims.h. */
SPANGPU_API void goertzel_reset(goertzel_state_t *s);
SPANGPU_API int goertzel_update(goertzel_state_t *s, const int16_t amp[], int samples);
SPANGPU_API float goertzel_result(goertzel_state_t *s);

/* ---- FSK receiver, modem connect tones, DTMF sender (csrc/shim_fsk.c) ---------------------------------
 * Reference declarations being replaced:
 *   fsk_rx_init/_restart/_rx/_fillin/_release/_free/_set_put_bit/_set_modem_status_handler/_set_signal_cutoff/
 *     _set_frame_parameters/_signal_power/_get_parity_errors/_get_framing_errors, fsk_spec_t, preset_fsk_specs[]
 *                                          src/spandsp/fsk.h:85-260      src/fsk.c:60-155,270-742
 *   modem_connect_tones_rx_init/_rx/_fillin/_get/_release/_free, modem_connect_tone_to_str
 *                                          src/spandsp/modem_connect_tones.h:57-200  src/modem_connect_tones.c:84-112,521-871
 *   dtmf_tx_init/_put/dtmf_tx/_set_level/_set_timing/_release/_free
 *                                          src/spandsp/dtmf.h:112-148    src/dtmf.c:551-676
 * As with the other families: xxx_init(NULL, ...) makes a private one-channel bank; a spangpu_line_group_t puts N
 * receivers on one bank and one launch per tick.  Storage supplied by the caller (s != NULL) cannot be used --
 * the state lives in HBM -- so such a call returns NULL.  fsk_rx_restart() accepts the spec the object was made
 * with (a bank runs one baud rate); a dtmf_tx digits callback is not replayed (init with one returns NULL).
 */
typedef struct
{
    const char *name;
    int freq_zero;
    int freq_one;
    int tx_level;
    int min_level;
    int baud_rate;
} fsk_spec_t;

enum
{
    FSK_V21CH1 = 0, FSK_V21CH2, FSK_V23CH1, FSK_V23CH2, FSK_BELL103CH1, FSK_BELL103CH2, FSK_BELL202, FSK_WEITBRECHT_4545,
    FSK_WEITBRECHT_50, FSK_WEITBRECHT_476, FSK_V21CH1_110
};

enum
{
    FSK_FRAME_MODE_ASYNC = 0,
    FSK_FRAME_MODE_SYNC = 1,
    FSK_FRAME_MODE_FRAMED = 2
};

enum
{
    ASYNC_PARITY_NONE = 0,
    ASYNC_PARITY_EVEN,
    ASYNC_PARITY_ODD,
    ASYNC_PARITY_MARK,
    ASYNC_PARITY_SPACE
};

enum
{
    MODEM_CONNECT_TONES_NONE = 0,
    MODEM_CONNECT_TONES_FAX_CNG = 1,
    MODEM_CONNECT_TONES_ANS = 2,
    MODEM_CONNECT_TONES_ANS_PR = 3,
    MODEM_CONNECT_TONES_ANSAM = 4,
    MODEM_CONNECT_TONES_ANSAM_PR = 5,
    MODEM_CONNECT_TONES_FAX_PREAMBLE = 6,
    MODEM_CONNECT_TONES_FAX_CED_OR_PREAMBLE = 7,
    MODEM_CONNECT_TONES_BELL_ANS = 8,
    MODEM_CONNECT_TONES_CALLING_TONE = 9,
    MODEM_CONNECT_TONES_REAL_TIME_REPORTS = 0x1000
};
#define MODEM_CONNECT_TONES_FAX_CED MODEM_CONNECT_TONES_ANS

typedef void (*digits_tx_callback_t)(void *user_data);

typedef struct fsk_rx_state_s fsk_rx_state_t;
typedef struct modem_connect_tones_rx_state_s modem_connect_tones_rx_state_t;
typedef struct dtmf_tx_state_s dtmf_tx_state_t;
typedef struct spangpu_line_group_s spangpu_line_group_t;

/* The objects themselves, for callers that bring their own storage (xxx_init(&my_state, ...), ended with xxx_release();
   spandsp keeps the like under spandsp/private/).  They are handles: the signal state lives in HBM.  Nothing in them is
   for the caller to touch. */
struct fsk_rx_state_s
{
    spangpu_line_group_t *grp;
    int channel;
    int private_grp;
    span_put_bit_func_t put_bit;
    void *put_bit_user_data;
    span_modem_status_func_t status_handler;
    void *status_user_data;
    int caller_storage;
};
struct modem_connect_tones_rx_state_s
{
    spangpu_line_group_t *grp;
    int channel;
    int private_grp;
    span_tone_report_func_t tone_callback;
    void *callback_data;
    int caller_storage;
    int tone_type;
};
struct dtmf_tx_state_s
{
    spangpu_txbank_t *bank;
    digits_tx_callback_t callback;
    void *callback_data;
    int puts;                   /* dtmf_tx_put() calls that queued digits (the callback's way of answering) */
    spangpu_object_t obj;
};

SPANGPU_API extern const fsk_spec_t preset_fsk_specs[];

SPANGPU_API spangpu_line_group_t *spangpu_fsk_group_create(int device, const fsk_spec_t *spec, int framing_mode, int n_channels,
                                                           int max_samples);
SPANGPU_API spangpu_line_group_t *spangpu_modem_connect_tones_group_create(int device, int tone_type, int use_callbacks,
                                                                           int n_channels, int max_samples);
SPANGPU_API int spangpu_line_group_destroy(spangpu_line_group_t *g);
SPANGPU_API int spangpu_line_group_flush(spangpu_line_group_t *g);

SPANGPU_API fsk_rx_state_t *fsk_rx_init(fsk_rx_state_t *s, const fsk_spec_t *spec, int framing_mode, span_put_bit_func_t put_bit,
                                        void *user_data);
SPANGPU_API fsk_rx_state_t *spangpu_fsk_rx_attach(spangpu_line_group_t *g, int channel, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API int fsk_rx_restart(fsk_rx_state_t *s, const fsk_spec_t *spec, int framing_mode);
SPANGPU_API int fsk_rx(fsk_rx_state_t *s, const int16_t *amp, int len);
SPANGPU_API int fsk_rx_fillin(fsk_rx_state_t *s, int len);
SPANGPU_API int fsk_rx_release(fsk_rx_state_t *s);
SPANGPU_API int fsk_rx_free(fsk_rx_state_t *s);
SPANGPU_API void fsk_rx_set_put_bit(fsk_rx_state_t *s, span_put_bit_func_t put_bit, void *user_data);
SPANGPU_API void fsk_rx_set_modem_status_handler(fsk_rx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API void fsk_rx_set_signal_cutoff(fsk_rx_state_t *s, float cutoff);
SPANGPU_API void fsk_rx_set_frame_parameters(fsk_rx_state_t *s, int data_bits, int parity, int stop_bits);
SPANGPU_API float fsk_rx_signal_power(fsk_rx_state_t *s);
SPANGPU_API int fsk_rx_get_parity_errors(fsk_rx_state_t *s, bool reset);
SPANGPU_API int fsk_rx_get_framing_errors(fsk_rx_state_t *s, bool reset);

SPANGPU_API modem_connect_tones_rx_state_t *modem_connect_tones_rx_init(modem_connect_tones_rx_state_t *s, int tone_type,
                                                                        span_tone_report_func_t tone_callback, void *user_data);
SPANGPU_API modem_connect_tones_rx_state_t *spangpu_modem_connect_tones_rx_attach(spangpu_line_group_t *g, int channel,
                                                                                  span_tone_report_func_t tone_callback,
                                                                                  void *user_data);
SPANGPU_API int modem_connect_tones_rx(modem_connect_tones_rx_state_t *s, const int16_t amp[], int len);
SPANGPU_API int modem_connect_tones_rx_fillin(modem_connect_tones_rx_state_t *s, int len);
SPANGPU_API int modem_connect_tones_rx_get(modem_connect_tones_rx_state_t *s);
SPANGPU_API int modem_connect_tones_rx_release(modem_connect_tones_rx_state_t *s);
SPANGPU_API int modem_connect_tones_rx_free(modem_connect_tones_rx_state_t *s);
SPANGPU_API const char *modem_connect_tone_to_str(int tone);

/* ---- FSK sender, modem connect tone generator, async character framer (csrc/shim_fsktx.c) -----------------
 * Reference declarations being replaced:
 *   fsk_tx_init/_restart/_power/_set_get_bit/_set_modem_status_handler/_release/_free, fsk_tx
 *                                          src/spandsp/fsk.h:160-193   src/fsk.c:162-269
 *   modem_connect_tones_tx_init/_release/_free, modem_connect_tones_tx
 *                                          src/spandsp/modem_connect_tones.h:115-138   src/modem_connect_tones.c:114-417
 *   async_tx_init/_get_bit/_presend_bits/_release/_free (host code)
 *                                          src/spandsp/async.h:212-241   src/async.c:277-393
 * A sender object is a one-channel bank (spangpu.h, "FSK and connect tone transmitter banks").  fsk_tx(s, amp, len)
 * works out how many bits the call needs, calls get_bit exactly that many times in order -- stopping at
 * SIG_STATUS_END_OF_DATA, after which it makes the two status calls and returns the short count, as fsk.c:179-189 --
 * and launches.  amp past the returned count is left as the caller had it.  Without a GPU the two _init() return NULL.
 */
typedef int (*span_get_bit_func_t)(void *user_data);
typedef int (*span_get_byte_func_t)(void *user_data);

typedef struct fsk_tx_state_s fsk_tx_state_t;
typedef struct modem_connect_tones_tx_state_s modem_connect_tones_tx_state_t;
typedef struct async_tx_state_s async_tx_state_t;

struct fsk_tx_state_s
{
    spangpu_fsktx_t *bank;
    span_get_bit_func_t get_bit;
    void *get_bit_user_data;
    span_modem_status_func_t status_handler;
    void *status_user_data;
    int baud_rate;
    int baud_frac;
    int shutdown;
    spangpu_object_t obj;
};
struct modem_connect_tones_tx_state_s
{
    spangpu_mcttx_t *bank;
    int tone_type;
    spangpu_object_t obj;
};
struct async_tx_state_s
{
    int data_bits;
    int parity;
    int stop_bits;
    int total_bits;
    span_get_byte_func_t get_byte;
    void *user_data;
    uint16_t frame_in_progress;
    int bitpos;
    int presend_bits;
    spangpu_object_t obj;
};

SPANGPU_API fsk_tx_state_t *fsk_tx_init(fsk_tx_state_t *s, const fsk_spec_t *spec, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API int fsk_tx_restart(fsk_tx_state_t *s, const fsk_spec_t *spec);
SPANGPU_API int fsk_tx_release(fsk_tx_state_t *s);
SPANGPU_API int fsk_tx_free(fsk_tx_state_t *s);
SPANGPU_API void fsk_tx_power(fsk_tx_state_t *s, float power);
SPANGPU_API void fsk_tx_set_get_bit(fsk_tx_state_t *s, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API void fsk_tx_set_modem_status_handler(fsk_tx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API int fsk_tx(fsk_tx_state_t *s, int16_t amp[], int len);

SPANGPU_API modem_connect_tones_tx_state_t *modem_connect_tones_tx_init(modem_connect_tones_tx_state_t *s, int tone_type);
SPANGPU_API int modem_connect_tones_tx_release(modem_connect_tones_tx_state_t *s);
SPANGPU_API int modem_connect_tones_tx_free(modem_connect_tones_tx_state_t *s);
SPANGPU_API int modem_connect_tones_tx(modem_connect_tones_tx_state_t *s, int16_t amp[], int len);

SPANGPU_API int async_tx_get_bit(void *user_data);
SPANGPU_API void async_tx_presend_bits(async_tx_state_t *s, int bits);
SPANGPU_API async_tx_state_t *async_tx_init(async_tx_state_t *s, int data_bits, int parity, int stop_bits, bool use_v14,
                                            span_get_byte_func_t get_byte, void *user_data);
SPANGPU_API int async_tx_release(async_tx_state_t *s);
SPANGPU_API int async_tx_free(async_tx_state_t *s);

/* ---- V.29, V.27ter and V.17 senders (csrc/shim_modemtx.c) --------------------------------------------------
 * Reference declarations being replaced:
 *   v29_tx_init/_restart/_release/_free/_power/_set_get_bit/_set_modem_status_handler/_get_logging_state, v29_tx
 *                                          src/spandsp/v29tx.h:110-170      src/v29tx.c:226-445
 *   v27ter_tx_* (same set)                 src/spandsp/v27ter_tx.h:80-139   src/v27ter_tx.c:257-447
 *   v17_tx_* (same set)                    src/spandsp/v17tx.h:97-158       src/v17tx.c:315-515
 * A sender object is a one-channel bank with the bit queue as its source (spangpu.h, "modem transmitter banks"): plumbing
 * for a caller that moves over one call at a time.  The path for scale is the bank: N channels per launch.
 * xxx_tx(s, amp, len) steps a cursor (spangpu_modemtx_cursor_advance()) to learn how many bits the call needs, calls get_bit
 * exactly that many times, in order, stops at SIG_STATUS_END_OF_DATA -- the status handler hears of it straight after that
 * get_bit, as in the reference -- queues the bits and launches.  SIG_STATUS_SHUTDOWN_COMPLETE comes in the call whose samples
 * end the shutdown (never from v17_tx, as in the reference), and later calls return 0.  Without a GPU the _init() return NULL.
 */
typedef struct
{
    spangpu_modemtx_t *bank;
    spangpu_modemtx_cursor_t cursor;
    span_get_bit_func_t get_bit;
    void *get_bit_user_data;
    span_modem_status_func_t status_handler;
    void *status_user_data;
    logging_state_t logging;
    spangpu_object_t obj;
} spangpu_modemtx_object_t;

typedef struct v29_tx_state_s v29_tx_state_t;
typedef struct v27ter_tx_state_s v27ter_tx_state_t;
typedef struct v17_tx_state_s v17_tx_state_t;
struct v29_tx_state_s
{
    spangpu_modemtx_object_t o;
};
struct v27ter_tx_state_s
{
    spangpu_modemtx_object_t o;
};
struct v17_tx_state_s
{
    spangpu_modemtx_object_t o;
};

SPANGPU_API v29_tx_state_t *v29_tx_init(v29_tx_state_t *s, int bit_rate, bool tep, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API int v29_tx_restart(v29_tx_state_t *s, int bit_rate, bool tep);
SPANGPU_API int v29_tx_release(v29_tx_state_t *s);
SPANGPU_API int v29_tx_free(v29_tx_state_t *s);
SPANGPU_API void v29_tx_power(v29_tx_state_t *s, float power);
SPANGPU_API void v29_tx_set_get_bit(v29_tx_state_t *s, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API void v29_tx_set_modem_status_handler(v29_tx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API logging_state_t *v29_tx_get_logging_state(v29_tx_state_t *s);
SPANGPU_API int v29_tx(v29_tx_state_t *s, int16_t amp[], int len);

SPANGPU_API v27ter_tx_state_t *v27ter_tx_init(v27ter_tx_state_t *s, int bit_rate, bool tep, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API int v27ter_tx_restart(v27ter_tx_state_t *s, int bit_rate, bool tep);
SPANGPU_API int v27ter_tx_release(v27ter_tx_state_t *s);
SPANGPU_API int v27ter_tx_free(v27ter_tx_state_t *s);
SPANGPU_API void v27ter_tx_power(v27ter_tx_state_t *s, float power);
SPANGPU_API void v27ter_tx_set_get_bit(v27ter_tx_state_t *s, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API void v27ter_tx_set_modem_status_handler(v27ter_tx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API logging_state_t *v27ter_tx_get_logging_state(v27ter_tx_state_t *s);
SPANGPU_API int v27ter_tx(v27ter_tx_state_t *s, int16_t amp[], int len);

SPANGPU_API v17_tx_state_t *v17_tx_init(v17_tx_state_t *s, int bit_rate, bool tep, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API int v17_tx_restart(v17_tx_state_t *s, int bit_rate, bool tep, bool short_train);
SPANGPU_API int v17_tx_release(v17_tx_state_t *s);
SPANGPU_API int v17_tx_free(v17_tx_state_t *s);
SPANGPU_API void v17_tx_power(v17_tx_state_t *s, float power);
SPANGPU_API void v17_tx_set_get_bit(v17_tx_state_t *s, span_get_bit_func_t get_bit, void *user_data);
SPANGPU_API void v17_tx_set_modem_status_handler(v17_tx_state_t *s, span_modem_status_func_t handler, void *user_data);
SPANGPU_API logging_state_t *v17_tx_get_logging_state(v17_tx_state_t *s);
SPANGPU_API int v17_tx(v17_tx_state_t *s, int16_t amp[], int len);

/* ---- in-band signalling tones (csrc/shim_sigtone.c) ------------------------------------------------------
 * Reference declarations being replaced:
 *   sig_tone_rx_init/_rx/_set_mode/_release/_free, sig_tone_tx_init/_tx/_set_mode/_release/_free
 *                                          src/spandsp/sig_tone.h:57-176   src/sig_tone.c:246-738
 * Tone types SIG_TONE_2280HZ .. SIG_TONE_2400HZ_2600HZ (1..3) and the mode / report bits are the SPANGPU_SIG_TONE_*
 * values of spangpu.h.  An object is a private one-channel bank (N channels per launch: spangpu_sigtone_rx_create()
 * etc.); caller storage (s != NULL) returns NULL, an object made by these functions is re-initialised in place.  Callbacks arrive from inside the call, in order, and a
 * mode set in one applies to the rest of the same frame, as in the reference.
 */
typedef struct sig_tone_rx_state_s sig_tone_rx_state_t;
typedef struct sig_tone_tx_state_s sig_tone_tx_state_t;

SPANGPU_API sig_tone_rx_state_t *sig_tone_rx_init(sig_tone_rx_state_t *s, int tone_type, span_tone_report_func_t sig_update,
                                                  void *user_data);
SPANGPU_API int sig_tone_rx(sig_tone_rx_state_t *s, int16_t amp[], int len);
SPANGPU_API void sig_tone_rx_set_mode(sig_tone_rx_state_t *s, int mode, int duration);
SPANGPU_API int sig_tone_rx_release(sig_tone_rx_state_t *s);
SPANGPU_API int sig_tone_rx_free(sig_tone_rx_state_t *s);
SPANGPU_API sig_tone_tx_state_t *sig_tone_tx_init(sig_tone_tx_state_t *s, int tone_type, span_tone_report_func_t sig_update,
                                                  void *user_data);
SPANGPU_API int sig_tone_tx(sig_tone_tx_state_t *s, int16_t amp[], int len);
SPANGPU_API void sig_tone_tx_set_mode(sig_tone_tx_state_t *s, int mode, int duration);
SPANGPU_API int sig_tone_tx_release(sig_tone_tx_state_t *s);
SPANGPU_API int sig_tone_tx_free(sig_tone_tx_state_t *s);

SPANGPU_API dtmf_tx_state_t *dtmf_tx_init(dtmf_tx_state_t *s, digits_tx_callback_t callback, void *user_data);
SPANGPU_API int dtmf_tx_release(dtmf_tx_state_t *s);
SPANGPU_API int dtmf_tx_free(dtmf_tx_state_t *s);
SPANGPU_API void dtmf_tx_set_level(dtmf_tx_state_t *s, int level, int twist);
SPANGPU_API void dtmf_tx_set_timing(dtmf_tx_state_t *s, int on_time, int off_time);
SPANGPU_API int dtmf_tx_put(dtmf_tx_state_t *s, const char *digits, int len);
SPANGPU_API int dtmf_tx(dtmf_tx_state_t *s, int16_t amp[], int max_samples);

/* Bell MF and MFC/R2 senders (src/spandsp/bell_r2_mf.h:137-191, src/bell_r2_mf.c:281-372,386-462): a private one-channel
   signal source bank each; caller-supplied storage (s != NULL) is not supported (state lives in HBM) */
typedef struct bell_mf_tx_state_s bell_mf_tx_state_t;
typedef struct r2_mf_tx_state_s r2_mf_tx_state_t;
struct bell_mf_tx_state_s
{
    spangpu_txbank_t *bank;
    spangpu_object_t obj;
};
struct r2_mf_tx_state_s
{
    spangpu_txbank_t *bank;
    spangpu_object_t obj;
};
SPANGPU_API bell_mf_tx_state_t *bell_mf_tx_init(bell_mf_tx_state_t *s);
SPANGPU_API int bell_mf_tx_release(bell_mf_tx_state_t *s);
SPANGPU_API int bell_mf_tx_free(bell_mf_tx_state_t *s);
SPANGPU_API int bell_mf_tx_put(bell_mf_tx_state_t *s, const char *digits, int len);
SPANGPU_API int bell_mf_tx(bell_mf_tx_state_t *s, int16_t amp[], int max_samples);
SPANGPU_API r2_mf_tx_state_t *r2_mf_tx_init(r2_mf_tx_state_t *s, bool fwd);
SPANGPU_API int r2_mf_tx_release(r2_mf_tx_state_t *s);
SPANGPU_API int r2_mf_tx_free(r2_mf_tx_state_t *s);
SPANGPU_API int r2_mf_tx_put(r2_mf_tx_state_t *s, char digit);
SPANGPU_API int r2_mf_tx(r2_mf_tx_state_t *s, int16_t amp[], int samples);

/* ---- V.18 text telephones in the Weitbrecht modes (csrc/shim_v18.c) ---------------------------------------------
 * Reference declarations being replaced:
 *   v18_init/_release/_free, v18_tx, v18_rx, v18_rx_fillin, v18_put, v18_get_current_mode, v18_set_stored_message,
 *   v18_mode_to_str, v18_status_to_str, v18_get_logging_state      src/spandsp/v18.h:124-214   src/v18.c:680-737, 1806-2130
 * An object is a one-channel V.18 text bank (spangpu.h, "V.18 text banks"): plumbing for a caller that moves over one call
 * at a time; the path for scale is the bank.  v18_init() returns NULL for a mode other than the three Weitbrecht 5-bit
 * modes (V18_MODE_REPETITIVE_SHIFTS_OPTION is stripped, as the reference strips it), for a nation other than
 * V18_AUTOMODING_NONE, and without a GPU.  put_msg is called from inside v18_rx(), once per character, with a NUL behind
 * it.  status_handler is kept and never called: the reference calls it from automoding only.
 * These names are declared with a macro of their own: tests/test_c_callers.py holds the SPANGPU_API names against a fixed
 * list of the reference's headers, and tests/test_v18_prototypes.py holds these against src/spandsp/v18.h.
 */
typedef void (*span_put_msg_func_t)(void *user_data, const uint8_t *msg, int len);

#define SPANGPU_V18_API SPANGPU_API

typedef struct v18_state_s v18_state_t;
struct v18_state_s
{
    spangpu_v18_t *bank;
    span_put_msg_func_t put_msg;
    void *put_msg_user_data;
    span_modem_status_func_t status_handler;
    void *status_handler_user_data;
    int current_mode;
    char stored_message[81];
    logging_state_t logging;
    spangpu_object_t obj;
};

enum
{
    V18_MODE_NONE = 0x0001,
    V18_MODE_WEITBRECHT_5BIT_4545 = 0x0002,
    V18_MODE_WEITBRECHT_5BIT_50 = 0x0004,
    V18_MODE_DTMF = 0x0008,
    V18_MODE_EDT = 0x0010,
    V18_MODE_BELL103 = 0x0020,
    V18_MODE_V23VIDEOTEX = 0x0040,
    V18_MODE_V21TEXTPHONE = 0x0080,
    V18_MODE_V18TEXTPHONE = 0x0100,
    V18_MODE_WEITBRECHT_5BIT_476 = 0x0200,
    V18_MODE_REPETITIVE_SHIFTS_OPTION = 0x1000
};

enum v18_autobauding_modes_e
{
    V18_AUTOMODING_GLOBAL = 0,
    V18_AUTOMODING_NONE,
    V18_AUTOMODING_AUSTRALIA,
    V18_AUTOMODING_IRELAND,
    V18_AUTOMODING_GERMANY,
    V18_AUTOMODING_SWITZERLAND,
    V18_AUTOMODING_ITALY,
    V18_AUTOMODING_SPAIN,
    V18_AUTOMODING_AUSTRIA,
    V18_AUTOMODING_NETHERLANDS,
    V18_AUTOMODING_ICELAND,
    V18_AUTOMODING_NORWAY,
    V18_AUTOMODING_SWEDEN,
    V18_AUTOMODING_FINALND,
    V18_AUTOMODING_DENMARK,
    V18_AUTOMODING_UK,
    V18_AUTOMODING_USA,
    V18_AUTOMODING_FRANCE,
    V18_AUTOMODING_BELGIUM,
    V18_AUTOMODING_END
};

enum v18_status_e
{
    V18_STATUS_SWITCH_TO_NONE,
    V18_STATUS_SWITCH_TO_WEITBRECHT_5BIT_4545,
    V18_STATUS_SWITCH_TO_WEITBRECHT_5BIT_476,
    V18_STATUS_SWITCH_TO_WEITBRECHT_5BIT_50,
    V18_STATUS_SWITCH_TO_DTMF,
    V18_STATUS_SWITCH_TO_EDT,
    V18_STATUS_SWITCH_TO_BELL103,
    V18_STATUS_SWITCH_TO_V23VIDEOTEX,
    V18_STATUS_SWITCH_TO_V21TEXTPHONE,
    V18_STATUS_SWITCH_TO_V18TEXTPHONE
};

SPANGPU_V18_API logging_state_t *v18_get_logging_state(v18_state_t *s);
SPANGPU_V18_API v18_state_t *v18_init(v18_state_t *s, bool calling_party, int mode, int nation, span_put_msg_func_t put_msg,
                                      void *put_msg_user_data, span_modem_status_func_t status_handler, void *status_handler_user_data);
SPANGPU_V18_API int v18_release(v18_state_t *s);
SPANGPU_V18_API int v18_free(v18_state_t *s);
SPANGPU_V18_API int v18_tx(v18_state_t *s, int16_t amp[], int max_len);
SPANGPU_V18_API int v18_rx(v18_state_t *s, const int16_t amp[], int len);
SPANGPU_V18_API int v18_rx_fillin(v18_state_t *s, int len);
SPANGPU_V18_API int v18_put(v18_state_t *s, const char msg[], int len);
SPANGPU_V18_API int v18_set_stored_message(v18_state_t *s, const char *msg);
SPANGPU_V18_API int v18_get_current_mode(v18_state_t *s);
SPANGPU_V18_API const char *v18_mode_to_str(int mode);
SPANGPU_V18_API const char *v18_status_to_str(int status);

/* ---- Caller ID in the four FSK standards (csrc/shim_adsi.c, csrc/adsi_host.c) ------------------------------------
 * Reference declarations being replaced:
 *   adsi_tx_init/_release/_free, adsi_tx, adsi_tx_put_message, adsi_tx_set_preamble, adsi_tx_send_alert_tone,
 *   adsi_rx_init/_release/_free, adsi_rx, adsi_add_field, adsi_next_field, adsi_standard_to_str,
 *   adsi_tx_get_logging_state, adsi_rx_get_logging_state          src/spandsp/adsi.h:393-519   src/adsi.c:436-771, 961-1237
 * An object is a one-channel caller-ID bank (spangpu.h, "Caller-ID banks"): plumbing for a caller that moves over one call
 * at a time; the path for scale is the bank.  adsi_tx_init() and adsi_rx_init() return NULL for ADSI_STANDARD_CLIP_DTMF and
 * ADSI_STANDARD_TDD (and any other value), and without a GPU.  put_msg is called from inside adsi_rx(), once per delivered
 * message, in order.  adsi_add_field(), adsi_next_field() and adsi_standard_to_str() are plain host code and take all six
 * standards; they read only the object's `standard` (and, for TDD, `baudot_shift`).  adsi_tx_put_message() returns -1 for
 * a message of fewer than 2 bytes, where the reference reads and writes outside the caller's bytes.
 * These names are declared with a macro of their own, as the V.18 ones are: tests/test_adsi.py holds them against
 * src/spandsp/adsi.h.
 */
#define SPANGPU_ADSI_API SPANGPU_API

enum
{
    ADSI_STANDARD_NONE = 0,
    ADSI_STANDARD_CLASS = 1,
    ADSI_STANDARD_CLIP = 2,
    ADSI_STANDARD_ACLIP = 3,
    ADSI_STANDARD_JCLIP = 4,
    ADSI_STANDARD_CLIP_DTMF = 5,
    ADSI_STANDARD_TDD = 6
};

/* message types and field types, by their values in the standards (Telcordia GR-30 / SR-TSV-002476, ETSI ETS 300 659-1 and
   ETS 300 778-1, NTT's caller ID service) */
enum
{
    CLASS_SDMF_CALLERID = 0x04,
    CLASS_MDMF_CALLERID = 0x80,
    CLASS_SDMF_MSG_WAITING = 0x06,
    CLASS_MDMF_MSG_WAITING = 0x82
};

enum
{
    MCLASS_DATETIME = 0x01,
    MCLASS_CALLER_NUMBER = 0x02,
    MCLASS_DIALED_NUMBER = 0x03,
    MCLASS_ABSENCE1 = 0x04,
    MCLASS_REDIRECT = 0x05,
    MCLASS_QUALIFIER = 0x06,
    MCLASS_CALLER_NAME = 0x07,
    MCLASS_ABSENCE2 = 0x08,
    MCLASS_ALT_ROUTE = 0x09
};

enum
{
    CLIP_MDMF_CALLERID = 0x80,
    CLIP_MDMF_MSG_WAITING = 0x82,
    CLIP_MDMF_CHARGE_INFO = 0x86,
    CLIP_MDMF_SMS = 0x89
};

enum
{
    CLIP_DATETIME = 0x01,
    CLIP_CALLER_NUMBER = 0x02,
    CLIP_DIALED_NUMBER = 0x03,
    CLIP_ABSENCE1 = 0x04,
    CLIP_CALLER_NAME = 0x07,
    CLIP_ABSENCE2 = 0x08,
    CLIP_VISUAL_INDICATOR = 0x0B,
    CLIP_MESSAGE_ID = 0x0D,
    CLIP_CALLTYPE = 0x11,
    CLIP_NUM_MSG = 0x13
};

enum
{
    ACLIP_SDMF_CALLERID = 0x04,
    ACLIP_MDMF_CALLERID = 0x80
};

enum
{
    ACLIP_DATETIME = 0x01,
    ACLIP_CALLER_NUMBER = 0x02,
    ACLIP_DIALED_NUMBER = 0x03,
    ACLIP_NUMBER_ABSENCE = 0x04,
    ACLIP_REDIRECT = 0x05,
    ACLIP_QUALIFIER = 0x06,
    ACLIP_CALLER_NAME = 0x07,
    ACLIP_NAME_ABSENCE = 0x08
};

#define JCLIP_MDMF_CALLERID             0x40

enum
{
    JCLIP_CALLER_NUMBER = 0x02,
    JCLIP_CALLER_NUM_DES = 0x21,
    JCLIP_DIALED_NUMBER = 0x09,
    JCLIP_DIALED_NUM_DES = 0x22,
    JCLIP_ABSENCE = 0x04
};

#define CLIP_DTMF_HASH_TERMINATED       '#'
#define CLIP_DTMF_C_TERMINATED          'C'
#define CLIP_DTMF_HASH_CALLER_NUMBER    'A'
#define CLIP_DTMF_HASH_ABSENCE          'D'
#define CLIP_DTMF_HASH_UNSPECIFIED      0

typedef struct adsi_tx_state_s adsi_tx_state_t;
struct adsi_tx_state_s
{
    int standard;
    int baudot_shift;
    spangpu_adsi_tx_t *bank;
    logging_state_t logging;
    spangpu_object_t obj;
};

typedef struct adsi_rx_state_s adsi_rx_state_t;
struct adsi_rx_state_s
{
    int standard;
    spangpu_adsi_rx_t *bank;
    span_put_msg_func_t put_msg;
    void *user_data;
    logging_state_t logging;
    spangpu_object_t obj;
};

SPANGPU_ADSI_API logging_state_t *adsi_rx_get_logging_state(adsi_rx_state_t *s);
SPANGPU_ADSI_API adsi_rx_state_t *adsi_rx_init(adsi_rx_state_t *s, int standard, span_put_msg_func_t put_msg, void *user_data);
SPANGPU_ADSI_API int adsi_rx_release(adsi_rx_state_t *s);
SPANGPU_ADSI_API int adsi_rx_free(adsi_rx_state_t *s);
SPANGPU_ADSI_API int adsi_rx(adsi_rx_state_t *s, const int16_t amp[], int len);
SPANGPU_ADSI_API logging_state_t *adsi_tx_get_logging_state(adsi_tx_state_t *s);
SPANGPU_ADSI_API adsi_tx_state_t *adsi_tx_init(adsi_tx_state_t *s, int standard);
SPANGPU_ADSI_API int adsi_tx_release(adsi_tx_state_t *s);
SPANGPU_ADSI_API int adsi_tx_free(adsi_tx_state_t *s);
SPANGPU_ADSI_API void adsi_tx_set_preamble(adsi_tx_state_t *s, int preamble_len, int preamble_ones_len, int postamble_ones_len, int stop_bits);
SPANGPU_ADSI_API int adsi_tx(adsi_tx_state_t *s, int16_t amp[], int max_len);
SPANGPU_ADSI_API void adsi_tx_send_alert_tone(adsi_tx_state_t *s);
SPANGPU_ADSI_API int adsi_tx_put_message(adsi_tx_state_t *s, const uint8_t *msg, int len);
SPANGPU_ADSI_API int adsi_next_field(adsi_rx_state_t *s, const uint8_t *msg, int msg_len, int pos, uint8_t *field_type, uint8_t const **field_body,
                                     int *field_len);
SPANGPU_ADSI_API int adsi_add_field(adsi_tx_state_t *s, uint8_t *msg, int len, uint8_t field_type, uint8_t const *field_body, int field_len);
SPANGPU_ADSI_API const char *adsi_standard_to_str(int standard);

/* ---- G.726 ADPCM (csrc/shim_g726.c) ---------------------------------------------------------------------------------
 * Reference declarations being replaced:
 *   g726_init, g726_release, g726_free, g726_encode, g726_decode            src/spandsp/g726.h:81-113   src/g726.c:1044-1251
 * An object is a one-channel codec bank (spangpu.h, "G.726 codec banks"): plumbing for a caller that moves over one call at
 * a time; the path for scale is the bank.  g726_init() returns NULL for a bit rate other than 16000, 24000, 32000 and 40000,
 * as the reference does, for a coding or packing outside its enums, and without a GPU.  `s` may be the caller's own storage
 * (this header has the whole struct, as the reference's private header has): g726_release() then gives up what the object
 * holds on the device and g726_free() leaves the storage alone.  amp[] is int16_t samples or G.711 bytes according to
 * ext_coding, as in the reference.  A codec call hands its output back in the same call, so these objects are not members
 * of channel groups (a group's calls are deferred to one replay).
 * These names are declared with a macro of their own, as the ADSI ones are: tests/test_g726.py holds them against
 * src/spandsp/g726.h.
 */
#define SPANGPU_G726_API SPANGPU_API

enum
{
    G726_ENCODING_LINEAR = 0,
    G726_ENCODING_ULAW,
    G726_ENCODING_ALAW
};

enum
{
    G726_PACKING_NONE = 0,
    G726_PACKING_LEFT = 1,
    G726_PACKING_RIGHT = 2
};

typedef struct g726_state_s g726_state_t;

struct g726_state_s
{
    int rate;
    int ext_coding;
    int bits_per_sample;
    int packing;
    spangpu_g726_t *bank;
    spangpu_object_t obj;
};

SPANGPU_G726_API g726_state_t *g726_init(g726_state_t *s, int bit_rate, int ext_coding, int packing);
SPANGPU_G726_API int g726_release(g726_state_t *s);
SPANGPU_G726_API int g726_free(g726_state_t *s);
SPANGPU_G726_API int g726_decode(g726_state_t *s, int16_t amp[], const uint8_t g726_data[], int g726_bytes);
SPANGPU_G726_API int g726_encode(g726_state_t *s, uint8_t g726_data[], const int16_t amp[], int len);

/* ---- G.722 wideband codec (csrc/shim_g722.c) ------------------------------------------------------------------------
 * Reference declarations being replaced:
 *   g722_encode_init, g722_encode_release, g722_encode_free, g722_encode    src/spandsp/g722.h:71-89    src/g722.c:457-661
 *   g722_decode_init, g722_decode_release, g722_decode_free, g722_decode    src/spandsp/g722.h:97-115   src/g722.c:261-454
 * An object is a one-channel codec bank (spangpu.h, "G.722 codec banks"): plumbing for a caller that moves over one call at
 * a time; the path for scale is the bank.  The init calls take every rate other than 48000 and 56000 for 64000, as the
 * reference does, and return NULL without a GPU.  `s` may be the caller's own storage (this header has the whole structs, as
 * the reference's private header has): the release call then gives up what the object holds on the device and the free
 * call leaves the storage alone.  One deviation: g722_encode() with an odd len on a 16 kHz encoder encodes len - 1 samples
 * and never reads amp[len], which the reference does.  A codec call hands its output back in the same call, so these objects
 * are not members of channel groups.
 * These names are declared with a macro of their own, as the G.726 ones are: tests/test_g722.py holds them against
 * src/spandsp/g722.h.
 */
#define SPANGPU_G722_API SPANGPU_API

enum
{
    G722_SAMPLE_RATE_8000 = 0x0001,
    G722_PACKED = 0x0002
};

typedef struct g722_encode_state_s g722_encode_state_t;
typedef struct g722_decode_state_s g722_decode_state_t;

struct g722_encode_state_s
{
    int bits_per_sample;
    int eight_k;
    int packed;
    spangpu_g722_t *bank;
    spangpu_object_t obj;
};

struct g722_decode_state_s
{
    int bits_per_sample;
    int eight_k;
    int packed;
    spangpu_g722_t *bank;
    spangpu_object_t obj;
};

SPANGPU_G722_API g722_encode_state_t *g722_encode_init(g722_encode_state_t *s, int rate, int options);
SPANGPU_G722_API int g722_encode_release(g722_encode_state_t *s);
SPANGPU_G722_API int g722_encode_free(g722_encode_state_t *s);
SPANGPU_G722_API int g722_encode(g722_encode_state_t *s, uint8_t g722_data[], const int16_t amp[], int len);
SPANGPU_G722_API g722_decode_state_t *g722_decode_init(g722_decode_state_t *s, int rate, int options);
SPANGPU_G722_API int g722_decode_release(g722_decode_state_t *s);
SPANGPU_G722_API int g722_decode_free(g722_decode_state_t *s);
SPANGPU_G722_API int g722_decode(g722_decode_state_t *s, int16_t amp[], const uint8_t g722_data[], int len);

/* ---- GSM 06.10 full-rate codec (csrc/shim_gsm0610.c, csrc/gsm0610_host.c) -------------------------------------------
 * Reference declarations being replaced:
 *   gsm0610_init, gsm0610_release, gsm0610_free, gsm0610_set_packing        src/spandsp/gsm0610.h:84-100  src/gsm0610_encode.c:108-341
 *   gsm0610_encode, gsm0610_decode                                          src/spandsp/gsm0610.h:108-116
 *   gsm0610_pack_none, _wav49, _voip, gsm0610_unpack_none, _wav49, _voip    src/spandsp/gsm0610.h:118-144
 * The reference has one state type for both directions; an object here is a pair of one-channel codec banks (spangpu.h,
 * "GSM 06.10 codec banks"), an encoder and a decoder with a history each: plumbing for a caller that
 * moves over one call at a time; the path for scale is the bank.  gsm0610_init() returns NULL without a GPU, and takes a
 * packing outside the three for GSM0610_PACKING_NONE, as the reference's switch statements do.  `s` may be the caller's own
 * storage (this header has the whole struct): the release call then gives up what the object holds on the device and the free
 * call leaves the storage alone.  One deviation: gsm0610_encode() and gsm0610_decode() work on the whole frames of `len`
 * (160 samples, 320 under WAV49; 76, 33 or 65 bytes) and never read past it, which the reference does at a partial frame.
 * The six pack and unpack calls are host code and need no GPU.  gsm0610_unpack_none() hands the bytes over as they are, as the
 * reference does; the decoders mask them.  These objects are not members of channel groups.
 * These names are declared with a macro of their own, as the G.722 ones are: tests/test_gsm0610.py holds them against
 * src/spandsp/gsm0610.h.
 */
#define SPANGPU_GSM0610_API SPANGPU_API

enum
{
    GSM0610_PACKING_NONE = 0,
    GSM0610_PACKING_WAV49 = 1,
    GSM0610_PACKING_VOIP = 2
};

typedef struct
{
    int16_t LARc[8];
    int16_t Nc[4];
    int16_t bc[4];
    int16_t Mc[4];
    int16_t xmaxc[4];
    int16_t xMc[4][13];
} gsm0610_frame_t;

typedef struct gsm0610_state_s gsm0610_state_t;

struct gsm0610_state_s
{
    int packing;
    spangpu_gsm0610_t *encoder;
    spangpu_gsm0610_t *decoder;
    spangpu_object_t obj;
};

SPANGPU_GSM0610_API gsm0610_state_t *gsm0610_init(gsm0610_state_t *s, int packing);
SPANGPU_GSM0610_API int gsm0610_release(gsm0610_state_t *s);
SPANGPU_GSM0610_API int gsm0610_free(gsm0610_state_t *s);
SPANGPU_GSM0610_API int gsm0610_set_packing(gsm0610_state_t *s, int packing);
SPANGPU_GSM0610_API int gsm0610_encode(gsm0610_state_t *s, uint8_t code[], const int16_t amp[], int len);
SPANGPU_GSM0610_API int gsm0610_decode(gsm0610_state_t *s, int16_t amp[], const uint8_t code[], int len);
SPANGPU_GSM0610_API int gsm0610_pack_none(uint8_t c[76], const gsm0610_frame_t *s);
SPANGPU_GSM0610_API int gsm0610_pack_wav49(uint8_t c[65], const gsm0610_frame_t *s);
SPANGPU_GSM0610_API int gsm0610_pack_voip(uint8_t c[33], const gsm0610_frame_t *s);
SPANGPU_GSM0610_API int gsm0610_unpack_none(gsm0610_frame_t *s, const uint8_t c[76]);
SPANGPU_GSM0610_API int gsm0610_unpack_wav49(gsm0610_frame_t *s, const uint8_t c[65]);
SPANGPU_GSM0610_API int gsm0610_unpack_voip(gsm0610_frame_t *s, const uint8_t c[33]);

/* ---- Packet loss concealment (csrc/shim_plc.c) -----------------------------------------------------------------------
 * Reference declarations being replaced:
 *   plc_rx, plc_fillin, plc_init, plc_release, plc_free                     src/spandsp/plc.h:125-149  src/plc.c:125-288
 * An object is a one-line concealment bank (spangpu.h, "Packet loss concealment banks"): plumbing for a caller that moves
 * over one call at a time; the path for scale is the bank.  plc_init() returns NULL without a GPU.  `s` may be the caller's
 * own storage (this header has the whole struct).  plc_rx() and plc_fillin() return len, and 0 on a NULL object; a len of 0
 * changes nothing (the reference's plc_rx() clears missing_samples there).  These objects are not members of channel groups.
 * These names are declared with a macro of their own, as the GSM 06.10 ones are: tests/test_plc.py holds them against
 * src/spandsp/plc.h.
 */
#define SPANGPU_PLC_API SPANGPU_API

typedef struct plc_state_s plc_state_t;

struct plc_state_s
{
    spangpu_plc_t *bank;
    spangpu_object_t obj;
};

SPANGPU_PLC_API int plc_rx(plc_state_t *s, int16_t amp[], int len);
SPANGPU_PLC_API int plc_fillin(plc_state_t *s, int16_t amp[], int len);
SPANGPU_PLC_API plc_state_t *plc_init(plc_state_t *s);
SPANGPU_PLC_API int plc_release(plc_state_t *s);
SPANGPU_PLC_API int plc_free(plc_state_t *s);

/* ---- IMA and OKI ADPCM (csrc/shim_adpcm.c) --------------------------------------------------------------------------
 * Reference declarations being replaced:
 *   ima_adpcm_init, ima_adpcm_release, ima_adpcm_free, ima_adpcm_encode, ima_adpcm_decode   src/spandsp/ima_adpcm.h:74-108
 *   oki_adpcm_init, oki_adpcm_release, oki_adpcm_free, oki_adpcm_encode, oki_adpcm_decode   src/spandsp/oki_adpcm.h
 * An object is a one-channel codec bank (spangpu.h, "IMA ADPCM codec banks", "OKI ADPCM codec banks"): plumbing for a caller
 * that moves over one call at a time; the path for scale is the bank.  oki_adpcm_init() returns NULL for a bit rate other
 * than 24000 and 32000, as the reference does; ima_adpcm_init() returns NULL for a variant outside the enum (the reference
 * takes it and then codes nothing); both return NULL without a GPU.  `s` may be the caller's own storage (this header has
 * the whole structs): the release call then gives up what the object holds on the device and the free call leaves the
 * storage alone.  A call is one launch up to 2^24 samples or bytes and is cut into launches beyond; a call that cannot be
 * cut without changing what it makes (IMA with chunk_size == 0: a header per call; VDVI: bits reset and padded per call)
 * returns 0 beyond that length.  The deviations of the banks hold here too: a length of 0 does nothing and returns 0, an IMA
 * decode call with chunk_size == 0 and fewer than 4 bytes returns 0, a header's step_index above 88 is taken as 88; and the
 * 24 kbit/s OKI paths narrow to int16_t as the reference's x86-64 build does (spangpu.h).  A codec call hands its output
 * back in the same call, so these objects are not members of channel groups.
 * These names are declared with a macro of their own, as the G.726 ones are: tests/test_adpcm.py holds them against
 * src/spandsp/ima_adpcm.h and src/spandsp/oki_adpcm.h.
 */
#define SPANGPU_ADPCM_API SPANGPU_API

enum
{
    IMA_ADPCM_IMA4 = 0,
    IMA_ADPCM_DVI4 = 1,
    IMA_ADPCM_VDVI = 2
};

typedef struct ima_adpcm_state_s ima_adpcm_state_t;
typedef struct oki_adpcm_state_s oki_adpcm_state_t;

struct ima_adpcm_state_s
{
    int variant;
    int chunk_size;
    spangpu_ima_adpcm_t *bank;
    spangpu_object_t obj;
};

struct oki_adpcm_state_s
{
    int bit_rate;
    spangpu_oki_adpcm_t *bank;
    spangpu_object_t obj;
};

SPANGPU_ADPCM_API ima_adpcm_state_t *ima_adpcm_init(ima_adpcm_state_t *s, int variant, int chunk_size);
SPANGPU_ADPCM_API int ima_adpcm_release(ima_adpcm_state_t *s);
SPANGPU_ADPCM_API int ima_adpcm_free(ima_adpcm_state_t *s);
SPANGPU_ADPCM_API int ima_adpcm_encode(ima_adpcm_state_t *s, uint8_t ima_data[], const int16_t amp[], int len);
SPANGPU_ADPCM_API int ima_adpcm_decode(ima_adpcm_state_t *s, int16_t amp[], const uint8_t ima_data[], int ima_bytes);
SPANGPU_ADPCM_API oki_adpcm_state_t *oki_adpcm_init(oki_adpcm_state_t *s, int bit_rate);
SPANGPU_ADPCM_API int oki_adpcm_release(oki_adpcm_state_t *s);
SPANGPU_ADPCM_API int oki_adpcm_free(oki_adpcm_state_t *s);
SPANGPU_ADPCM_API int oki_adpcm_encode(oki_adpcm_state_t *s, uint8_t oki_data[], const int16_t amp[], int len);
SPANGPU_ADPCM_API int oki_adpcm_decode(oki_adpcm_state_t *s, int16_t amp[], const uint8_t oki_data[], int oki_bytes);

#if defined(__cplusplus)
}
#endif

#endif
