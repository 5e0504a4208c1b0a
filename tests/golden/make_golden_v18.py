"""Writes tests/golden/v18_weitbrecht.npz from the live reference (oracle/_ref/libspandsp_ref.so and the reference's headers):

  offsets       [field][offset, size] of the v18_state_t fields tests/v18_ref.py reads (v18_ref.FIELDS), measured by a C
                compiler on the reference's own private header;
  per mode m    text_m, and for a sender given that text and run in 160-sample calls to its end with a second reference
                object listening: tx_m [calls][160] samples, len_m [calls] returned lengths, far_m / far_at_m the characters
                the far end printed and the call each was printed in; codes_m the 5-bit codes on the line.

Run from the repository root:  python tests/golden/make_golden_v18.py [reference source dir]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_LRINT", "-DHAVE_LRINTF", "-DHAVE_STDLIB_H", "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H",
        "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LONG_DOUBLE"]
TEXT = b"Hello, World 123! ok"


def measure_offsets(ref_src, fields):
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <math.h>",
             "#include <stdbool.h>"]
    for h in ("telephony", "alloc", "logging", "fast_convert", "queue", "async", "complex", "dds", "tone_detect", "tone_generate",
              "super_tone_rx", "power_meter", "fsk", "dtmf", "modem_connect_tones", "v8", "v18", "private/logging", "private/queue",
              "private/tone_generate", "private/async", "private/power_meter", "private/fsk", "private/dtmf",
              "private/modem_connect_tones", "private/v18"):
        lines.append('#include "spandsp/%s.h"' % h)
    lines += [
             "int main(void) {"]
    for f in fields:
        lines.append('printf("%%zu %%zu\\n", offsetof(v18_state_t, %s), sizeof(((v18_state_t *) 0)->%s));' % (f, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "off.c")
        open(src, "w").write("\n".join(lines) + "\n")
        exe = os.path.join(d, "off")
        subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32)


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    import v18_ref
    out = {"offsets": measure_offsets(ref_src, v18_ref.FIELDS)}
    np.savez_compressed(v18_ref.GOLDEN, **out)      # RefV18.field() reads the offsets from the file
    v18_ref._golden.clear()
    for mode in v18_ref.MODES:
        near = v18_ref.RefV18(mode)
        far = v18_ref.RefV18(mode)
        assert near.put(TEXT) == len(TEXT)
        rows, lens, far_text, far_at, own = [], [], b"", [], b""
        for call in range(4000):
            row, got = near.tx(160)
            full = np.zeros(160, np.int16)
            full[:got] = row[:got]
            rows.append(full)
            lens.append(got)
            own += near.rx(full)
            printed = far.rx(full)
            far_text += printed
            far_at += [call]*len(printed)
            if got < 160:
                break
        assert own == b"" and far_text == TEXT.upper(), (own, far_text)
        m = "%04x" % mode
        out["text_" + m] = np.frombuffer(TEXT, np.uint8)
        out["tx_" + m] = np.array(rows, np.int16)
        out["len_" + m] = np.array(lens, np.int32)
        out["far_" + m] = np.frombuffer(far_text, np.uint8)
        out["far_at_" + m] = np.array(far_at, np.int32)
        out["codes_" + m] = v18_ref.line_codes(mode, np.concatenate(rows))
        print(m, len(lens), "calls, last", lens[-1], far_text)
    np.savez_compressed(v18_ref.GOLDEN, **out)
    print("wrote", v18_ref.GOLDEN, os.path.getsize(v18_ref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
