"""Writes tests/golden/subsegments.npz: what the reference's own kaldi/utils/data/get_uniform_subsegments.py prints for a segments file
that hits its float and rounding quirks, under the option sets tests/test_subsegments_host.py checks libs.amd.subsegments against.

Needs the reference tree (build container only); the script is run as a subprocess under this interpreter, with the command line
pytorch/pipeline/extract_xvectors_for_pytorch.sh:72-77 gives it: --overlap-duration is what `perl -e "print ($window-$period)"`
prints, i.e. '%.15g'.  --constant-duration is an argparse `type=bool`: any non-empty text is True, so the False case leaves it out.
The fixture holds data only: the input lines, the option sets and the printed lines."""

import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
SCRIPT = os.path.join(REF, "kaldi", "utils", "data", "get_uniform_subsegments.py")

# (window, period, min_segment, constant_duration): the shell script's defaults, a longer window, and the script's own default of
# --constant-duration
OPTION_SETS = [(1.5, 0.75, 0.5, True), (3.0, 1.0, 0.5, True), (1.5, 0.75, 0.5, False)]


def segments():
    """(utt, rec, start, end): start times whose binary form is not exact, durations around every threshold of the cut."""
    rows = []

    def add(start, dur):
        rows.append(("utt%02d" % len(rows), "rec%d" % (len(rows) % 3), start, start + dur))

    for start in (0.0, 0.07, 0.29, 10.5):
        for dur in (1.5, 1.51, 4.10):                      # exactly one window, a hundredth more, a few windows and a remainder
            add(start, dur)
    for dur in (0.01, 0.3, 0.49, 0.5):                      # below (and at) min_segment
        add(0.0, dur)
    for dur in (1.99, 2.0, 2.01, 2.24, 2.25, 2.26, 2.74, 2.75, 2.76):      # window + min_segment -+ 0.01, and around one period more
        add(0.29, dur)
    for dur in (3.0, 3.01, 3.49, 3.5, 3.51, 7.3):           # the same for the 3.0 s window
        add(10.5, dur)
    add(123.45, 33.33)
    add(0.0, 600.0)                                         # ten minutes: ~800 windows; the sums drift
    add(0.07, 0.75)
    return rows


def main():
    if not os.path.isfile(SCRIPT):
        sys.exit("gen_subsegments_golden.py needs the reference tree at %s (build container only)" % REF)
    lines = ["%s %s %s %s" % (u, r, repr(round(s, 2)), repr(round(e, 2))) for u, r, s, e in segments()]
    out = {"segments": np.array(lines), "option_sets": np.array(OPTION_SETS, dtype=np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "segments")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        for k, (window, period, min_segment, constant) in enumerate(OPTION_SETS):
            cmd = [sys.executable, SCRIPT, "--max-segment-duration=%s" % window, "--overlap-duration=%.15g" % (window - period),
                   "--max-remaining-duration=%s" % min_segment]
            if constant:
                cmd.append("--constant-duration=True")
            printed = subprocess.run(cmd + [path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
            out["lines_%d" % k] = np.array(printed.splitlines())
            print("option set %d %r: %d lines" % (k, OPTION_SETS[k], len(out["lines_%d" % k])))
    dst = os.path.join(REPO, "tests", "golden", "subsegments.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
