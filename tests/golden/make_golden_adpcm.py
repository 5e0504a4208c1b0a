"""Writes tests/golden/ima_adpcm.npz and tests/golden/oki_adpcm.npz from the live reference.  ima_adpcm.c, oki_adpcm.c and
alloc.c are compiled here, in a temporary directory, with the flags of oracle/Makefile (STRICT + DEFS); they link on their
own, and nothing compiled is kept.  The fixtures hold data only; the lines and the reference's driver come from
tests/adpcm_lines.py.

  line, line_crc      the encoders' line (int16) and its CRC-32;
  schedule            the call lengths cycled by every stream that may be cut anywhere;
  offsets             [word][offset, size] of the state type's fields the banks' state words map to, in that order, measured
                      by a compiler on the reference's private header;
  index               [case][family, 0 encoder / 1 decoder, variant or bit rate, chunk size, 0 line / 1 random / 2 phase1, may be
                      recut, OKI's `phase` before the first call];
  data<i>             a decoder's bytes (an encoder's input is `line`);
  want<i>             what the case makes;
  calls<i>            [call][length, count, the state words after it].

Per configuration: the encoder on the line, the decoder of what it made, and a decoder on random bytes.  A decoder whose
calls are packets (chunk_size == 0, VDVI) takes the encoder's calls one for one; under a header its random line has a header
with a step_index inside the table in front of every call.  The generator asserts that the lines reach what
adpcm_lines.coverage_ima() / coverage_oki() name.

Run from the repository root:  python tests/golden/make_golden_adpcm.py [reference source dir]"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import adpcm_lines as al  # noqa: E402


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = al.build_reference(ref_src, d)
        assert L.oki_adpcm_init(None, 16000) is None and L.oki_adpcm_init(None, 40000) is None
        for family in (al.IMA, al.OKI):
            cs = []
            for a, b in al.CONFIGS[family]:
                cs += list(al.reference_cases(L, offsets, family, a, b, al.line(), "line"))
                noise, lens = al.random_packets(family, a, b)
                cs.append(al.run_reference(L, offsets, family, al.DECODE, a, b, "rnd", noise, lens, not al.is_packets(family, a, b)))
            if family == al.OKI:
                # a decoder that begins at phase 1 (see coverage_oki())
                noise, lens = al.random_packets(family, 24000, 0)
                cs.append(al.run_reference(L, offsets, family, al.DECODE, 24000, 0, "phase1", noise[:300], al.calls(300), True, entry_phase=1))
            got = al.COVERAGE[family](cs)
            for name, ok in got.items():
                print("%-9s %-60s %s" % (al.NAMES[family], name, "reached" if ok else "MISSING"))
            missing = [n for n, ok in got.items() if not ok]
            assert not missing, "no line shows %s: lengthen or reseed a line in tests/adpcm_lines.py" % missing
            out = al.store(cs)
            out["offsets"] = offsets[family]
            path = os.path.join(HERE, al.NAMES[family] + ".npz")
            np.savez_compressed(path, **out)
            print("wrote", path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) <= 478071
            # what was written reads back as the same cases
            back = al.cases(al.load(family, path))
            assert len(back) == len(cs) and all(np.array_equal(x.want, y.want) and x.name == y.name for x, y in zip(back, cs))


if __name__ == "__main__":
    main()
