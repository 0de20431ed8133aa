#!/bin/bash
# Proves that a source clean-up left the device code alone: compiles csrc/*.hip of a base revision and of the working tree to gfx950 assembly with the
# Makefile's HIPFLAGS, drops the lines that name the per-compile __hip_cuid symbol and compares the rest byte for byte. It only diffs; no GPU needed.
# Checks the .hip files that differ from the base, or every .hip file when a header differs. One line per file; exit status 1 if any file differs.
# usage: scripts/device_code_identity.sh <base revision> [csrc file name ...]
set -euo pipefail
base=${1:?usage: $0 <base revision> [csrc file name ...]}; shift
root=$(cd "$(dirname "$0")/.." && pwd)
proj=neural-color-transfer_amd
cd "$root"
tmp=$(mktemp -d)
trap 'git worktree remove --force "$tmp/base" 2>/dev/null || true; rm -rf "$tmp"' EXIT
git worktree add --detach "$tmp/base" "$base" >/dev/null 2>&1
hipcc=$(make -s -C $proj --eval='print-hipcc: ; @echo $(HIPCC)' print-hipcc)
flags=$(make -s -C $proj --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags)

if [ $# -gt 0 ]; then files="$*"
elif ! git diff --quiet "$base" -- include "$proj/csrc/*.h"; then files=$(cd $proj/csrc && ls *.hip)
else files=$(git diff --name-only "$base" -- "$proj/csrc/*.hip" | xargs -r -n1 basename)
fi
[ -n "$files" ] || { echo "no .hip file differs from $base"; exit 0; }

asm() {     # <tree> <file> <output>: device assembly without the __hip_cuid lines; the compiler's messages only if it fails
    (cd "$1/$proj" && $hipcc $flags --cuda-device-only -S "csrc/$2" -o - 2>"$3.err" | grep -v __hip_cuid > "$3") || { cat "$3.err" >&2; return 1; }
}
status=0
for f in $files; do
    [ -f "$tmp/base/$proj/csrc/$f" ] || { echo "$f: not in $base"; status=1; continue; }
    asm "$tmp/base" "$f" "$tmp/$f.base.s" & p0=$!
    asm "$root" "$f" "$tmp/$f.new.s" & p1=$!
    wait $p0; wait $p1
    if cmp -s "$tmp/$f.base.s" "$tmp/$f.new.s"; then echo "$f: identical ($(wc -l < "$tmp/$f.new.s") lines)"
    else echo "$f: DIFFERS"; status=1; fi
done
exit $status
