"""Writes tests/golden/loud_modems.npz from the live reference (oracle/_ref): every (modem, bit rate, line) of
tests/loud_modem_lines.py through the reference's receivers on the uneven call schedule, un-rotated, and the lost-packet
cases of xxx_rx_fillin().  Data only.

  keys                 the case names, sorted: "rx/<modem>_<rate>/<line>" and "fillin/<modem>_<rate>/<point>"
  line_crcs            CRC-32 of the 17 lines and of every rate's own_x8 and own_x40 (loud_modem_lines.line_crcs())
  <family>.<field>.data / .shape   the field of all the family's cases back to back, and each case's shape

  rx      call_crcs: CRC-32 of the put_bit / status values (int8) of every call, 0 for a call that gave none;
          status: the negative values in order; sums [bits delivered, CRC-32 of the whole stream];
          fwords (bit patterns), iwords: the state words at the end
  fillin  a committed clean transmission (tests/golden/<modem>_<rate>.npz) on 160-sample calls, the first n samples of one
          call replaced by xxx_rx_fillin(n): at [the call, n]; events: the whole stream; fwords_after, iwords_after: the
          state words right after the fill-in; fwords, iwords: at the end.  Points: "start" (call 0, no signal: a no-op),
          "training", "data" (after TRAINING_SUCCEEDED), "parked" (the sine2280 line after TRAINING_FAILED: a no-op), all
          with n = 160; "training_97", "data_97" with n = 97

The same lines give the same bytes: the archive carries no time stamps.

Run from the repository root:  python tests/golden/make_golden_loud_modems.py [output file]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import loud_lines as ll  # noqa: E402
import loud_modem_lines as lm  # noqa: E402


def main():
    import oracle
    assert oracle.have_ref(), "oracle/_ref is not built: the fixture comes from the reference"
    path = sys.argv[1] if len(sys.argv) > 1 else lm.GOLDEN
    cases = lm.all_cases(lm.receivers("ref"), lm.ref_fillin)
    ll.write_archive(path, lm.pack(cases))
    print("wrote", path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
