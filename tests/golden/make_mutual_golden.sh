#!/bin/sh
# Mints the known answers of the mutual-coverage search (tests/test_gpu_mutual_cover_seed.py, tests/test_length_ratio_core.py):
# ext_mutual_{fast,default,sensitive,hashed}.tap = the reference's stage-2 seed hits and Match lists per query (seam: Extension::extend,
# oracle/ref_tap.cpp) with --min-len-ratio 0.75 on the inputs of tests/mutual_sets.py. The reference length-sorts both blocks
# first, so the blocks in the tap header are the sorted ones. Needs oracle/_ref/diamond_tap (make -C oracle).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
TAP="$ROOT/oracle/_ref/diamond_tap"
TMP="$(mktemp -d)"
DMND_ROOT="$ROOT" python3 - "$TMP" <<'PY'
import os, sys
sys.path.insert(0, os.environ["DMND_ROOT"]); sys.path.insert(0, os.path.join(os.environ["DMND_ROOT"], "tests"))
from diamond_amd import synth
import mutual_sets
# (the near-identical families give the default mode's deferred pass pairs whose batch loses a mate to the length test)
for tag, kw in (("fast", dict(families=40, members=5, queries=2, seed=31)), ("default", dict(families=24, members=5, queries=2, near=3, seed=32)),
                ("sensitive", dict(families=14, members=4, queries=2, near=1, near_members=6, near_queries=2, seed=33, hi=360))):
    db, do, q, qo = mutual_sets.generate(**kw)
    synth.write_fasta("%s/%s_db.faa" % (sys.argv[1], tag), "t", db, do)
    synth.write_fasta("%s/%s_q.faa" % (sys.argv[1], tag), "q", q, qo)
PY
for tag in fast default sensitive; do
  mode="--$tag"; [ "$tag" = default ] && mode=""
  DIAMOND_TAP_EXT="$HERE/ext_mutual_$tag.tap" \
    "$TAP" blastp $mode --min-len-ratio 0.75 --masking 0 --motif-masking 0 --algo 0 -k 0 -q "$TMP/${tag}_q.faa" -d "$TMP/${tag}_db.faa" -o "$TMP/$tag.out" -p1 2>/dev/null
done
# the query-indexed algorithm (hashed seed encoding) on the --fast inputs
DIAMOND_TAP_EXT="$HERE/ext_mutual_hashed.tap" \
  "$TAP" blastp --fast --min-len-ratio 0.75 --masking 0 --motif-masking 0 --algo 1 -k 0 -q "$TMP/fast_q.faa" -d "$TMP/fast_db.faa" -o "$TMP/hashed.out" -p1 2>/dev/null
ls -la "$HERE"/ext_mutual_*.tap
rm -rf "$TMP"
