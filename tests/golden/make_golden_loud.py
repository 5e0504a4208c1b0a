"""Writes tests/golden/loud_lines.npz from the live reference (oracle/_ref): every (configuration, line) of
tests/loud_lines.py through the reference's receivers on the uneven call schedule, cut down to what the fixture keeps.

  keys                 the case names, "<family>/<configuration>/<line>", sorted
  line_crcs            CRC-32 of every line as generated (loud_lines.line_crcs())
  <family>.<field>.data / .shape   the field of all the family's cases back to back, and each case's shape

  sigrx   reports [k][state, level, duration]; snaps: the state words after every tenth call and at the end;
          sums [CRC-32 of the rewritten line, its length, samples left on a rail where the input sample is another]
  sigtx   snaps; sums [CRC-32 of the line sent, its length, update requests, samples on a rail where the media is not]
  mct     reports [k][tone, level, 0]; hits: the latch read after every tenth call (latch form); snaps
  fsk     head: the first 64 put_bit values; final: the 28 scalar words at the end;
          sums [events, CRC-32 of them all, CRC-32 of the snapshots of every sixteenth call and the end, how many]
  echo    final: the control words at the end; sums [CRC-32 of the clean line, of the control words after every call, of
          taps32, taps16, history, clean samples on a rail where rx is not, max |taps32|]
  dtmf, bell, r2f, r2b, st   digits; final: filter state and counters at the end; sums [events, CRC-32 of them, CRC-32
          of the state after every call]

The same lines and configurations give the same bytes: the archive carries no time stamps.

Run from the repository root:  python tests/golden/make_golden_loud.py [output file]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import loud_lines as ll  # noqa: E402


def main():
    import oracle
    assert oracle.have_ref(), "oracle/_ref is not built: the fixture comes from the reference"
    path = sys.argv[1] if len(sys.argv) > 1 else ll.GOLDEN
    cases = ll.all_cases(ll.makers("ref"))
    ll.write_archive(path, ll.pack(cases))
    print("wrote", path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
