#!/bin/bash
# Is the device code of the tabular kernels the same as at another revision?  Compiles the gfx950
# assembly of each file from the working tree and from a `git archive` of REV (in a temporary
# directory) with the Makefile's flags, and prints one line per file: its hash on both sides and
# `same` or `DIFFERENT`.  The fixed -cuid matters: without it two builds of identical source differ.
#   bash scripts/device_code_diff.sh HEAD~1 [file.hip ...]
# Exit status 1 if any file differs.  A host-only change must leave every file `same`.
set -euo pipefail
REV=${1:?usage: device_code_diff.sh REV [file.hip ...]}
shift
FILES=${*:-tabular.hip tabular_pwg.hip tabular_nact.hip general.hip}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# (FLAGS of cobel-rl_amd/csrc/Makefile)
F="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -fvisibility=hidden -munsafe-fp-atomics -Wall -Wno-unused-function"
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/rev" "$TMP/out"
git -C "$ROOT" archive "$REV" cobel-rl_amd/csrc include | tar -x -C "$TMP/rev"
asm() {   # asm <tree> <file> <output>
  (cd "$1/cobel-rl_amd/csrc" && $HIPCC $F --offload-device-only -S -cuid=cobel "$2" -o "$3")
}
rc=0
for f in $FILES; do
  asm "$TMP/rev" "$f" "$TMP/out/rev_$f.s" &
  asm "$ROOT" "$f" "$TMP/out/tree_$f.s" &
done
wait
for f in $FILES; do
  a=$(sha256sum < "$TMP/out/rev_$f.s" | cut -c1-16)
  b=$(sha256sum < "$TMP/out/tree_$f.s" | cut -c1-16)
  if [ "$a" = "$b" ]; then v=same; else v=DIFFERENT; rc=1; fi
  printf '%-18s %s %s  %s  %s\n' "$f" "$REV" "$a" "$b" "$v"
  if [ -n "${KEEP_ASM:-}" ]; then cp "$TMP/out/rev_$f.s" "$TMP/out/tree_$f.s" "$KEEP_ASM/"; fi
done
exit $rc
