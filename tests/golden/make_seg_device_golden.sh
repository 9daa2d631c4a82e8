#!/bin/bash
# Golden of tests/test_seg_core.py and tests/test_gpu_seg.py: the reference's own SEG (oracle/_ref/seg_ref = src/lib/blast/blast_seg.cpp
# compiled in place behind oracle/seg_ref_main.cpp) on tests/golden/seg_device_cases.faa.gz -- the cases the device form of SEG can get
# wrong and the other SEG goldens never reach: segments whose trim cuts the trigger window off on the left, so that the left remainder is
# searched again (one of them with more than one segment in that search), overlapping neighbours, lengths around the window and around
# one and two wavefronts, windows with exactly two and three non-standard letters, a sequence of X only, and a homopolymer of 10 050
# letters (its raw segment is above the ln n! table: the device hands it back to the host).
# One line per sequence: id, then begin-end (0-based, inclusive) of every masked segment.
set -e
here="$(cd "$(dirname "$0")" && pwd)"
seg="$here/../../oracle/_ref/seg_ref"
zcat "$here/seg_device_cases.faa.gz" | "$seg" | gzip -9nc > "$here/seg_device_golden.tsv.gz"
