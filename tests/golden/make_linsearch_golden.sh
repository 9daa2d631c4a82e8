#!/bin/sh
# Mints the known answers of the linearised search (tests/test_gpu_linsearch_seed.py, tests/test_linsearch_core.py):
# ext_lin_{fast,default,hashed}.tap = the reference's stage-2 seed hits and Match lists per query (seam: Extension::extend,
# oracle/ref_tap.cpp) with --linsearch on inputs of tests/mutual_sets.py. The reference length-sorts the reference block first
# and leaves the query block as it is, so the tap header holds a sorted reference block and an unsorted query block.
# The default golden must hold hits with a window score above 255 (the near-identical families give them), and in each golden
# the first-position rule must drop at least 10 % of the joined reference positions: tests/test_linsearch_core.py asserts both,
# run it after minting. Needs oracle/_ref/diamond_tap (make -C oracle).
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
for tag, kw in (("fast", dict(families=30, members=5, queries=2, seed=61)), ("default", dict(families=18, members=5, queries=2, near=3, near_members=6, seed=62))):
    db, do, q, qo = mutual_sets.generate(**kw)
    synth.write_fasta("%s/%s_db.faa" % (sys.argv[1], tag), "t", db, do)
    synth.write_fasta("%s/%s_q.faa" % (sys.argv[1], tag), "q", q, qo)
PY
for tag in fast default; do
  mode="--$tag"; [ "$tag" = default ] && mode=""
  DIAMOND_TAP_EXT="$HERE/ext_lin_$tag.tap" \
    "$TAP" blastp $mode --linsearch --masking 0 --motif-masking 0 --algo 0 -k 0 -q "$TMP/${tag}_q.faa" -d "$TMP/${tag}_db.faa" -o "$TMP/$tag.out" -p1 2>/dev/null
done
# the query-indexed algorithm (hashed seed encoding) on the --fast inputs
DIAMOND_TAP_EXT="$HERE/ext_lin_hashed.tap" \
  "$TAP" blastp --fast --linsearch --masking 0 --motif-masking 0 --algo 1 -k 0 -q "$TMP/fast_q.faa" -d "$TMP/fast_db.faa" -o "$TMP/hashed.out" -p1 2>/dev/null
ls -la "$HERE"/ext_lin_*.tap
rm -rf "$TMP"
