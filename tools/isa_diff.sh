#!/bin/bash
# tools/isa_diff.sh TREE_A TREE_B: is the gfx950 device code of every csrc/tg_*.hip the same in two checkouts?
# Each file is compiled to assembly (device side only) with its own tree's build.sh flags and `// TG_FILE_FLAGS:` line;
# assembler comments and directives (first non-blank character `;` or `.`) and the per-translation-unit __hip_cuid_*
# symbol are dropped, the rest -- every label and instruction -- is diffed.  Exit status 1 on any difference.
# JOBS=n compiles n files at a time (default 8); FILES="tg_a.hip tg_b.hip" restricts the comparison to those files.
set -euo pipefail
[ $# = 2 ] || { echo "usage: $0 <tree A> <tree B>" >&2; exit 2; }
export HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SUB=tecogan-pytorch_amd/csrc
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
asm_one() {  # <csrc dir> <out dir> <file>: the filtered instruction stream of one source
  local flags ff
  flags=$(sed -n 's/^FLAGS="\(.*\)"$/\1/p' "$1/build.sh" | head -1)
  ff=$(sed -n 's/^\/\/ TG_FILE_FLAGS: *//p' "$1/$3" | head -1)
  (cd "$1" && $HIPCC $flags $ff -Wno-unused-command-line-argument --cuda-device-only -S "$3" -o -) | { grep -v '^[[:space:]]*[;.]\|__hip_cuid_' || true; } > "$2/${3%.hip}.s"
}
export -f asm_one
for t in A B; do
  [ $t = A ] && d="$1/$SUB" || d="$2/$SUB"
  mkdir "$TMP/$t"
  (cd "$d" && ls ${FILES:-tg_*.hip}) | xargs -P "${JOBS:-8}" -I{} bash -c 'set -euo pipefail; asm_one "$@"' _ "$(cd "$d" && pwd)" "$TMP/$t" {}
done
rc=0
for f in $( (cd "$TMP/A" && ls; cd "$TMP/B" && ls) | sort -u ); do
  if ! diff -q "$TMP/A/$f" "$TMP/B/$f" > /dev/null 2>&1; then
    echo "DIFFERENT: ${f%.s}.hip ($(diff "$TMP/A/$f" "$TMP/B/$f" 2>&1 | grep -c '^[<>]' || true) lines)"
    rc=1
  fi
done
[ $rc = 0 ] && echo "identical: $(ls "$TMP/A" | wc -l) files"
exit $rc
