"""Writes tests/golden/adsi_fsk.npz from the live reference.  adsi.c and crc.c are not among the modules of
oracle/_ref/libspandsp_ref.so, so the two files are compiled here, in a temporary directory, with the flags of oracle/Makefile
(STRICT + DEFS), linked against that library, and nothing compiled is kept.  The fixture holds only what adsi.c produced:

  offsets           [field][offset, size] of the adsi_tx_state_t (TX_FIELDS) and adsi_rx_state_t (RX_FIELDS) fields the banks'
                    state words map to, measured by a compiler on the reference's private header;
  pack_*            per standard and message of adsi_lines.FIELD_CASES: the adsi_add_field()-built message, the sender's
                    msg[] after adsi_tx_put_message(), the adsi_next_field() walk (pos, type, len, body offset per step, the
                    terminating return last); also add_field on CLIP-DTMF and TDD;
  tx_<run>_<std>    sender runs on fsktx_ref.SCHEDULE's call lengths, cycled: samples (what was produced, concatenated),
                    returned lengths, state words after each call; runs: plain, alert (adsi_tx_send_alert_tone() before the
                    put), preamble (adsi_tx_set_preamble(s, 40, 20, 7, 2)), second (a put while busy, then a second message
                    after the first has ended); the too-long returns;
  rx_<line>         for every line of tests/adsi_lines.py: the messages delivered, the call each arrived in, framing_errors
                    and the final state words.

Run from the repository root:  python tests/golden/make_golden_adsi.py [reference source dir]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import adsi_lines as AL     # noqa: E402
import fsktx_ref            # noqa: E402

GOLDEN = os.path.join(HERE, "adsi_fsk.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
# the order of the banks' state words (adsi_dev.hpp: ADT_*, then FT_BAUD_RATE .. FT_SHUTDOWN; ADR_*)
TX_FIELDS = ("standard", "preamble_len", "preamble_ones_len", "postamble_ones_len", "stop_bits", "byte_no", "bit_pos", "bit_no", "msg_len",
             "tx_signal_on", "alert_tone_gen.current_section", "alert_tone_gen.current_position", "alert_tone_gen.phase[0]",
             "alert_tone_gen.phase[1]", "alert_tone_gen.duration[0]", "alert_tone_gen.duration[1]", "fsk_tx.baud_rate",
             "fsk_tx.phase_rates[0]", "fsk_tx.phase_rates[1]", "fsk_tx.scaling", "fsk_tx.current_phase_rate", "fsk_tx.phase_acc",
             "fsk_tx.baud_frac", "fsk_tx.shutdown", "msg")
RX_FIELDS = ("standard", "consecutive_ones", "bit_pos", "in_progress", "msg_len", "framing_errors", "msg")
PUT_MSG = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_int)
HEADERS = ("telephony", "alloc", "fast_convert", "logging", "queue", "complex", "dds", "power_meter", "async", "crc", "fsk", "tone_detect",
           "tone_generate", "super_tone_rx", "dtmf", "adsi", "private/logging", "private/queue", "private/tone_generate", "private/async",
           "private/power_meter", "private/fsk", "private/dtmf", "private/adsi")


def build_reference(ref_src, d):
    """adsi.c + crc.c as a shared object beside the checker library, and the offsets program"""
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(d, "libadsi_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, "-shared", "-o", so,
                    os.path.join(ref_src, "adsi.c"), os.path.join(ref_src, "crc.c"), "-L" + ref_dir, "-lspandsp_ref",
                    "-Wl,-rpath," + ref_dir, "-lm"], check=True)
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <math.h>",
             "#include <stdbool.h>"] + ['#include "spandsp/%s.h"' % h for h in HEADERS] + ["int main(void) {"]
    for typ, fields in (("adsi_tx_state_t", TX_FIELDS), ("adsi_rx_state_t", RX_FIELDS)):
        for f in fields:
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *) 0)->%s));' % (typ, f, typ, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32)
    fsktx_ref.lib()
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in [("adsi_tx_init", vp, [vp, ci]), ("adsi_tx_free", ci, [vp]), ("adsi_tx", ci, [vp, vp, ci]),
                            ("adsi_tx_put_message", ci, [vp, C.c_char_p, ci]), ("adsi_tx_set_preamble", None, [vp, ci, ci, ci, ci]),
                            ("adsi_tx_send_alert_tone", None, [vp]), ("adsi_rx_init", vp, [vp, ci, vp, vp]), ("adsi_rx_free", ci, [vp]),
                            ("adsi_rx", ci, [vp, vp, ci]),
                            ("adsi_add_field", ci, [vp, vp, ci, C.c_uint8, C.c_char_p, ci]),
                            ("adsi_next_field", ci, [vp, vp, ci, ci, C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(ci)])]:
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L, offsets


class Ref:
    def __init__(self, L, offsets):
        self.L = L
        self.tx_off = offsets[:len(TX_FIELDS)]
        self.rx_off = offsets[len(TX_FIELDS):]

    def words(self, p, offs, n):
        out = []
        for off, size in offs[:n]:
            out.append(int.from_bytes(C.string_at(p + int(off), int(size)), "little", signed=True))
        return np.array([w & 0xFFFFFFFF for w in out], np.uint32).view(np.int32)

    def tx_words(self, p):
        return self.words(p, self.tx_off, len(TX_FIELDS) - 1)

    def tx_msg(self, p):
        off = int(self.tx_off[-1][0])
        n = int(self.tx_words(p)[8])
        return np.frombuffer(C.string_at(p + off, n), np.uint8).copy()

    def rx_words(self, p):
        return self.words(p, self.rx_off, len(RX_FIELDS) - 1)

    def add_field(self, s, msg, t, body):
        buf = C.create_string_buffer(bytes(msg) + bytes(1024), 1024 + len(msg))
        n = self.L.adsi_add_field(s, buf, len(msg) if msg else -1, t, bytes(body), len(body))
        return buf.raw[:n]

    def walk(self, s, msg):
        """adsi_next_field() to its end: rows of (returned pos, type, len, body offset or -1); the last row is the end"""
        buf = C.create_string_buffer(bytes(msg), len(msg) + 8)
        base = C.addressof(buf)
        rows, pos = [], -1
        for _ in range(64):
            t, body, n = C.c_uint8(0), C.c_void_p(None), C.c_int(0)
            pos = self.L.adsi_next_field(s, base, len(msg), pos, C.byref(t), C.byref(body), C.byref(n))
            if pos < 0:
                rows.append((pos, 0, 0, -1))
                break
            rows.append((pos, t.value, n.value, (body.value - base) if body.value else -1))
        return np.array(rows, np.int32)

    def run_tx(self, s, calls=None, until_idle=True, limit=200):
        """adsi_tx() on SCHEDULE's lengths, cycled, until a call returns nothing (and two calls more)"""
        rows, lens, words, idle, k = [], [], [], 0, 0
        while k < limit:
            n = fsktx_ref.SCHEDULE[k % len(fsktx_ref.SCHEDULE)]
            row = np.zeros(n, np.int16)
            got = self.L.adsi_tx(s, row.ctypes.data, n)
            rows.append(row[:got].copy())
            lens.append(got)
            words.append(self.tx_words(s))
            k += 1
            idle = idle + 1 if got == 0 else 0
            if idle >= 2 or (calls is not None and k >= calls):
                break
        return rows, lens, words

    def run_rx(self, standard, samples, tick):
        got = []
        call = [0]
        cb = PUT_MSG(lambda _, msg, n: got.append((call[0], bytes(msg[:n]))))
        p = self.L.adsi_rx_init(None, standard, C.cast(cb, C.c_void_p), None)
        for k, row in enumerate(AL.calls_of(samples, tick)):
            call[0] = k
            self.L.adsi_rx(p, row.ctypes.data, len(row))
        words = self.rx_words(p)
        self.L.adsi_rx_free(p)
        return got, words


def pack_messages(got):
    """[(call, bytes)] as three arrays: calls, lengths, the bytes back to back"""
    return (np.array([c for c, _ in got], np.int32), np.array([len(m) for _, m in got], np.int32),
            np.frombuffer(b"".join(m for _, m in got), np.uint8).copy())


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        R = Ref(L, offsets)
        out = {"offsets": offsets}

        # ---- packing and fields ----
        for s in AL.STANDARDS + (5, 6):
            tx = L.adsi_tx_init(None, s)
            rx = L.adsi_rx_init(None, s, None, None)
            for case, fields in sorted(AL.FIELD_CASES.items()):
                if s > 4 and case != "cid":
                    continue
                fl = fields(AL.JCLIP if s == 4 else AL.CLASS)
                if s == 5:
                    fl = [(ord("#"), b""), (ord("A"), b"0123456789"), (0, b"4455")]
                if s == 6:
                    fl = [(0, b"Hello 123, ok? go"), (0, b"\n#9 z")]
                msg = b""
                for t, body in fl:
                    msg = R.add_field(tx, msg, t, body)
                key = "pack_%d_%s" % (s, case)
                out[key + "_msg"] = np.frombuffer(msg, np.uint8).copy()
                if s <= 4:
                    assert msg == AL.build(s, fl), (s, case)
                    fresh = L.adsi_tx_init(None, s)
                    assert L.adsi_tx_put_message(fresh, msg, len(msg)) == len(msg)
                    out[key + "_packed"] = R.tx_msg(fresh)
                    assert bytes(out[key + "_packed"]) == AL.pack(s, msg), (s, case)
                    L.adsi_tx_free(fresh)
                    # the walk is over what a receiver delivers: the packed bytes less the sum check / as they are for J-CLIP
                    seen = bytes(b & 0x7F for b in out[key + "_packed"]) if s == 4 else bytes(out[key + "_packed"][:-1])
                    out[key + "_seen"] = np.frombuffer(seen, np.uint8).copy()
                    out[key + "_walk"] = R.walk(rx, seen)
                else:
                    out[key + "_walk"] = R.walk(rx, msg)
            L.adsi_tx_free(tx)
            L.adsi_rx_free(rx)

        # ---- senders ----
        for s in AL.STANDARDS:
            msg = AL.sweep_message(s)
            other = AL.number_message(s, b"987", b"Zed")
            for run in ("plain", "alert", "preamble", "second"):
                tx = L.adsi_tx_init(None, s)
                first_words = R.tx_words(tx)
                if run == "alert":
                    L.adsi_tx_send_alert_tone(tx)
                if run == "preamble":
                    L.adsi_tx_set_preamble(tx, 40, 20, 7, 2)
                assert L.adsi_tx_put_message(tx, msg, len(msg)) == len(msg)
                key = "tx_%s_%d" % (run, s)
                if run == "second":
                    rows, lens, words = R.run_tx(tx, calls=4)
                    assert L.adsi_tx_put_message(tx, other, len(other)) == 0
                    r2, l2, w2 = R.run_tx(tx)
                    # (the schedule starts again with every run_tx: the test does the same)
                    assert L.adsi_tx_put_message(tx, other, len(other)) == len(other)
                    r3, l3, w3 = R.run_tx(tx)
                    out[key + "_split"] = np.array([len(lens), len(lens) + len(l2)], np.int32)
                    rows, lens, words = rows + r2 + r3, lens + l2 + l3, words + w2 + w3
                else:
                    rows, lens, words = R.run_tx(tx)
                if run == "plain":
                    # the Python restatement the receiver lines are rendered from, against the reference's own sender
                    mine = AL.render(s, AL.burst_bits(AL.pack(s, msg), AL.defaults(s)))
                    assert np.array_equal(mine, np.concatenate(rows)), s
                    out["tx_init_%d" % s] = first_words
                out[key + "_pcm"] = np.concatenate(rows)
                out[key + "_len"] = np.array(lens, np.int32)
                out[key + "_words"] = np.array(words, np.int32)
                print(key, len(lens), "calls", int(np.sum(lens)), "samples")
                L.adsi_tx_free(tx)
            tx = L.adsi_tx_init(None, s)
            longs = [119, 120] if s == 4 else [255, 256]
            res = []
            for n in longs:
                fresh = L.adsi_tx_init(None, s)
                res.append(L.adsi_tx_put_message(fresh, bytes((i*3 + 1) & 0x7F for i in range(n)), n))
                L.adsi_tx_free(fresh)
            out["tx_long_%d" % s] = np.array([longs, res], np.int32)
            assert res == [longs[0], -1], res
            L.adsi_tx_free(tx)

        # ---- receivers ----
        delivered = {}
        for name, s, samples in AL.sweep_lines():
            got, words = R.run_rx(s, samples, AL.TICK)
            delivered[name] = got
            att = int(name.split("_a")[1].split("_")[0])
            want = bytes(AL.pack(s, AL.sweep_message(s)))
            want = bytes(b & 0x7F for b in want[:-2]) if s == 4 else want[:-1]
            if att in AL.AUDIBLE:
                assert [m for _, m in got] == [want], (name, got)
            else:
                assert got == [], (name, got)
            out["rx_%s_at" % name], out["rx_%s_len" % name], out["rx_%s_bytes" % name] = pack_messages(got)
            out["rx_%s_words" % name] = words
        for name, s, samples, tick in AL.hand_lines():
            got, words = R.run_rx(s, samples, tick)
            out["rx_%s_at" % name], out["rx_%s_len" % name], out["rx_%s_bytes" % name] = pack_messages(got)
            out["rx_%s_words" % name] = words
            print(name, [(c, len(m)) for c, m in got], "framing errors", int(words[5]), "msg_len", int(words[4]))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
