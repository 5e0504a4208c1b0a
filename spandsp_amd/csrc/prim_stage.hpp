// prim_stage.hpp -- how the array arguments of the fourteen spangpu_*_batch() primitives (prim_api.hip, prim2_api.hip) lie in
// memory: ONE rule for which strides a call accepts and how many elements it touches, and ONE table of the arguments.  No
// HIP call and no include of HIP's: tests/c_callers/prim_extents.cpp drives this header alone, under -fsanitize=address,undefined
// (tests/test_prim_extents.py), and the entry points take every staging and copy-back count from here (prim_stage_hip.hpp).
//
// The rule, for an array of `items` rows of `row` elements, `stride` elements apart:
//   - stride 0 (one row for all items) only where the array may be shared, and never for an array the call writes;
//   - otherwise stride >= row (rows never overlap), and never negative;
//   - the extent -- row for a stride of 0, else stride*(items - 1) + row, 0 for a row of 0 -- times the element size fits in
//     size_t (checked in unsigned arithmetic; nothing here can overflow a signed type);
//   - the extent is what the call reads, stages, and (a written array) copies back: a caller's array need be no longer.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace spg
{

// false: the stride is not allowed (or the extent does not fit); *extent in elements otherwise
static inline bool prim_extent(long long row, long long stride, int items, bool may_share, bool written, size_t elem, size_t *extent)
{
    *extent = 0;
    if (row < 0  ||  stride < 0  ||  items <= 0  ||  elem == 0)
        return false;
    if (stride == 0)
    {
        if (!may_share  ||  written)
            return false;
    }
    else if (stride < row)
    {
        return false;
    }
    const size_t most = SIZE_MAX/elem;
    const size_t r = (size_t) row;
    const size_t s = (size_t) stride;
    const size_t m = (size_t) (items - 1);
    if (r > most  ||  (m != 0  &&  s > (most - r)/m))
        return false;
    *extent = (r == 0)  ?  0  :  s*m + r;
    return true;
}

// ---- the arguments ----------------------------------------------------------------------------------------------------

enum PrimRow
{
    kRowOne,        // one element an item
    kRowN,          // n (len) elements
    kRowHalf,       // len/2 elements
    kRowState,      // a Godard detector's 8 state words
    kRowDesc        // ... and its 12 descriptor words
};

enum PrimUse
{
    kIn,            // read
    kOut,           // written, every element of every row: nothing of the caller's goes to the device
    kInOut          // advanced in place
};

struct PrimArg
{
    const char *call;       // the entry point, without spangpu_ and _batch
    const char *name;
    PrimRow row;
    unsigned elem;          // bytes; a complex element is 8
    PrimUse use;
    bool may_share;         // stride 0 allowed
    bool strided;           // the call has a stride parameter for it; false: rows lie back to back (stride = row)
};

static inline long long prim_row(PrimRow row, int n)
{
    switch (row)
    {
    case kRowN:
        return n;
    case kRowHalf:
        return n/2;
    case kRowState:
        return 8;
    case kRowDesc:
        return 12;
    default:
        return 1;
    }
}

// the rule on an argument of the table; `stride` is looked at only where the call has one
static inline bool prim_arg_extent(const PrimArg &a, long long stride, int items, int n, size_t *extent)
{
    const long long row = prim_row(a.row, n);
    if (!a.strided)
    {
        // back to back: a row of 0 (nothing to touch) goes through the rule with a stride of 1
        stride = (row > 0)  ?  row  :  1;
    }
    return prim_extent(row, stride, items, a.may_share, a.use != kIn, a.elem, extent);
}

#define SPG_PRIM_ARG(id, call, name, row, elem, use, share, strided) constexpr PrimArg id = {call, name, row, elem, use, share, strided};

//           constant         call                        name          row        elem use     share  strided
#define SPG_PRIM_ARGS(X) \
    X(kVecDotX,      "vec_circular_dot_prodf",   "x",          kRowN,     4,   kIn,    true,  true)  \
    X(kVecDotY,      "vec_circular_dot_prodf",   "y",          kRowN,     4,   kIn,    true,  true)  \
    X(kVecDotPos,    "vec_circular_dot_prodf",   "pos",        kRowOne,   4,   kIn,    false, false) \
    X(kVecDotZ,      "vec_circular_dot_prodf",   "z",          kRowOne,   4,   kOut,   false, false) \
    X(kVecLmsX,      "vec_circular_lmsf",        "x",          kRowN,     4,   kIn,    true,  true)  \
    X(kVecLmsY,      "vec_circular_lmsf",        "y",          kRowN,     4,   kInOut, false, true)  \
    X(kVecLmsPos,    "vec_circular_lmsf",        "pos",        kRowOne,   4,   kIn,    false, false) \
    X(kVecLmsErr,    "vec_circular_lmsf",        "error",      kRowOne,   4,   kIn,    false, false) \
    X(kCvecDotX,     "cvec_circular_dot_prodf",  "x",          kRowN,     8,   kIn,    true,  true)  \
    X(kCvecDotY,     "cvec_circular_dot_prodf",  "y",          kRowN,     8,   kIn,    true,  true)  \
    X(kCvecDotPos,   "cvec_circular_dot_prodf",  "pos",        kRowOne,   4,   kIn,    false, false) \
    X(kCvecDotZ,     "cvec_circular_dot_prodf",  "z",          kRowOne,   8,   kOut,   false, false) \
    X(kCvecLmsX,     "cvec_circular_lmsf",       "x",          kRowN,     8,   kIn,    true,  true)  \
    X(kCvecLmsY,     "cvec_circular_lmsf",       "y",          kRowN,     8,   kInOut, false, true)  \
    X(kCvecLmsPos,   "cvec_circular_lmsf",       "pos",        kRowOne,   4,   kIn,    false, false) \
    X(kCvecLmsErr,   "cvec_circular_lmsf",       "error",      kRowOne,   8,   kIn,    false, false) \
    X(kPowerAmp,     "power_meter_update",       "amp",        kRowN,     2,   kIn,    true,  true)  \
    X(kPowerReading, "power_meter_update",       "reading",    kRowOne,   4,   kInOut, false, false) \
    X(kPowerShift,   "power_meter_update",       "shift",      kRowOne,   4,   kIn,    false, false) \
    X(kGodardRxState, "godard_ted_rx",           "state",      kRowState, 4,   kInOut, false, false) \
    X(kGodardRxDesc, "godard_ted_rx",            "desc",       kRowDesc,  4,   kIn,    true,  true)  \
    X(kGodardRxSamples, "godard_ted_rx",         "samples",    kRowN,     4,   kIn,    true,  true)  \
    X(kGodardBaudState, "godard_ted_per_baud",   "state",      kRowState, 4,   kInOut, false, false) \
    X(kGodardBaudDesc, "godard_ted_per_baud",    "desc",       kRowDesc,  4,   kIn,    true,  true)  \
    X(kGodardBaudCorr, "godard_ted_per_baud",    "correction", kRowOne,   4,   kOut,   false, false) \
    X(kPgramCoeffs,  "periodogram",              "coeffs",     kRowHalf,  8,   kIn,    true,  true)  \
    X(kPgramAmp,     "periodogram",              "amp",        kRowN,     8,   kIn,    true,  true)  \
    X(kPgramOut,     "periodogram",              "out",        kRowOne,   8,   kOut,   false, false) \
    X(kPrepAmp,      "periodogram_prepare",      "amp",        kRowN,     8,   kIn,    true,  true)  \
    X(kPrepSum,      "periodogram_prepare",      "sum",        kRowHalf,  8,   kOut,   false, false) \
    X(kPrepDiff,     "periodogram_prepare",      "diff",       kRowHalf,  8,   kOut,   false, false) \
    X(kApplyCoeffs,  "periodogram_apply",        "coeffs",     kRowHalf,  8,   kIn,    true,  true)  \
    X(kApplySum,     "periodogram_apply",        "sum",        kRowHalf,  8,   kIn,    false, false) \
    X(kApplyDiff,    "periodogram_apply",        "diff",       kRowHalf,  8,   kIn,    false, false) \
    X(kApplyOut,     "periodogram_apply",        "out",        kRowOne,   8,   kOut,   false, false) \
    X(kFreqErrLast,  "periodogram_freq_error",   "last_result", kRowOne,  8,   kIn,    false, false) \
    X(kFreqErrNow,   "periodogram_freq_error",   "result",     kRowOne,   8,   kIn,    false, false) \
    X(kFreqErrOut,   "periodogram_freq_error",   "out",        kRowOne,   4,   kOut,   false, false) \
    X(kSqrtX,        "fixed_sqrt32",             "x",          kRowOne,   4,   kIn,    false, false) \
    X(kSqrtOut,      "fixed_sqrt32",             "out",        kRowOne,   2,   kOut,   false, false) \
    X(kDdsAcc,       "dds_complexf",             "phase_acc",  kRowOne,   4,   kInOut, false, false) \
    X(kDdsRate,      "dds_complexf",             "phase_rate", kRowOne,   4,   kIn,    false, false) \
    X(kDdsOut,       "dds_complexf",             "out",        kRowN,     8,   kOut,   false, false) \
    X(kAtanY,        "arctan2",                  "y",          kRowOne,   4,   kIn,    false, false) \
    X(kAtanX,        "arctan2",                  "x",          kRowOne,   4,   kIn,    false, false) \
    X(kAtanOut,      "arctan2",                  "out",        kRowOne,   4,   kOut,   false, false)

SPG_PRIM_ARGS(SPG_PRIM_ARG)

// the same constants as one table (periodogram_freq_error's phase_offset is two floats in host memory whatever `mem` says:
// an argument by value, not an array of rows)
#define SPG_PRIM_ARG_ROW(id, call, name, row, elem, use, share, strided) id,
constexpr PrimArg kPrimArgs[] = { SPG_PRIM_ARGS(SPG_PRIM_ARG_ROW) };
constexpr int kPrimArgCount = (int) (sizeof(kPrimArgs)/sizeof(kPrimArgs[0]));

#undef SPG_PRIM_ARG_ROW
#undef SPG_PRIM_ARG

}   // namespace spg
