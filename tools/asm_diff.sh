#!/bin/bash
# tools/asm_diff.sh OLD_TREE NEW_TREE [FILE.hip ...]  -> per source file: "identical", or the symbols whose device assembly differs
# Compiles every file of the Makefile's SRCS (or the files named) in both trees to gfx950 assembly with the Makefile's flags, per-file flags
# included, and compares whole lines.  Only the __hip_cuid_<hash> symbol (a hash of the source text) is masked.  For a refactor that must
# not change a kernel: git worktree add /tmp/parent HEAD^ && tools/asm_diff.sh /tmp/parent .
# OUT=dir keeps the .s files there (default: a fresh temporary directory); JOBS=n compiles n files at a time (default 8).
# BY_SYMBOL=1: a file that differs as a whole is compared again symbol by symbol -- each function's lines, its kernel descriptor and its
# metadata entry under its name, the rest of the file in place, the function numbers in local labels (.LBB3_7) masked -- and passes as
# "same per symbol" if only the order in which the compiler emitted the functions changed (a host-side change can move an instantiation).
# A file that still differs gets three lists: the symbols that are identical, those that differ (with the number of differing lines) and
# those only one side has -- for a refactor that changes some kernels of a file and must leave the others alone.
set -e
old=$(realpath "$1"); new=$(realpath "$2"); shift 2
out=${OUT:-$(mktemp -d)}; mkdir -p "$out/old" "$out/new"
mk=$new/echoseal_amd/csrc/Makefile
srcs=${*:-$(sed -n 's/^SRCS *:= *//p' "$mk")}
flags=$(sed -n 's/^HIPFLAGS *?= *//p' "$mk" | sed 's/\$(ARCH)/gfx950/')

for side in old new; do
  for f in $srcs; do
    tree=$old; [ $side = new ] && tree=$new
    [ -f "$tree/echoseal_amd/csrc/$f" ] || continue
    per_file=$(sed -n "s/^FLAGS_${f%.hip} := //p" "$tree/echoseal_amd/csrc/Makefile")
    echo "cd $tree/echoseal_amd/csrc && /opt/rocm/bin/hipcc $flags $per_file -Wno-unused-command-line-argument --cuda-device-only -S $f -o $out/$side/${f%.hip}.s"
  done
done | xargs -P "${JOBS:-8}" -d '\n' -n 1 sh -c

# by_symbol FILE: every line under the symbol it belongs to, symbols sorted by name, lines of one symbol in file order
by_symbol() {
  sed -E 's/\.L(BB|JTI|CPI)[0-9]+_/.L\1_/g; s/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1/g; s/([= ])BB[0-9]+_/\1BB_/g' "$1" | awk '
    function flush(   i) { for (i = 0; i < n; ++i) print name "\t" buf[i]; n = 0; name = "" }
    /^\t\.text$/ { next }                                                       # (a bare section switch: present or not by what follows)
    /^\t\.p2alignl|^\t\.section\t\.AMDGPU\.gpr_maximums/ { sym = "~tail" }       # after the last function: padding, maxima, objects
    /^\t\.section\t\.text\./ { sym = $2; sub(/^\.text\./, "", sym); sub(/,.*/, "", sym) }
    /; -- Begin function / { sym = $NF }
    /^amdhsa\.kernels:/ { print "~meta\t" $0; meta = 1; next }
    meta && /^  - \./ { flush() }                                               # a kernel entry of the metadata: filed under its .name
    meta && /^amdhsa\.target:/ { flush(); meta = 0; sym = "~meta" }
    meta { buf[n++] = $0; if ($1 == ".name:") name = $2; next }
    { print sym "\t" $0 }' | sort -s -t "$(printf '\t')" -k1,1
}

status=0
for f in $srcs; do
  for side in old new; do
    sed 's/__hip_cuid_[0-9a-f]*/__hip_cuid_X/g' "$out/$side/${f%.hip}.s" > "$out/$side/${f%.hip}.masked"
  done
  if cmp -s "$out/old/${f%.hip}.masked" "$out/new/${f%.hip}.masked"; then
    echo "$f: identical ($(wc -l < "$out/new/${f%.hip}.s") lines)"
  elif [ -n "$BY_SYMBOL" ] && by_symbol "$out/old/${f%.hip}.masked" > "$out/old/${f%.hip}.sorted" && by_symbol "$out/new/${f%.hip}.masked" > "$out/new/${f%.hip}.sorted" &&
       cmp -s "$out/old/${f%.hip}.sorted" "$out/new/${f%.hip}.sorted"; then
    echo "$f: same per symbol, functions emitted in another order ($(grep -c -- '-- Begin function' "$out/new/${f%.hip}.s") functions)"
  elif [ -n "$BY_SYMBOL" ]; then
    # the per-symbol verdict, from the .sorted files: which symbols both sides have line for line, which differ (lines that differ, both
    # sides counted), which only one side has.  ~meta and ~tail are the file's own lines outside any function.
    status=1
    o=$out/old/${f%.hip}; n=$out/new/${f%.hip}
    cut -f1 "$o.sorted" | uniq > "$o.syms"; cut -f1 "$n.sorted" | uniq > "$n.syms"
    comm -12 "$o.syms" "$n.syms" > "$n.both"
    diff "$o.sorted" "$n.sorted" | sed -n 's/^[<>] \([^\t]*\)\t.*/\1/p' | sort | uniq -c | awk '{ print $2 "\t" $1 }' | sort -t "$(printf '\t')" -k1,1 | join -t "$(printf '\t')" - "$n.both" > "$n.differing" || true
    cut -f1 "$n.differing" | comm -13 - "$n.both" > "$n.identical"
    echo "$f: DIFFERS per symbol"
    echo "  identical ($(wc -l < "$n.identical")):"; sed 's/^$/(before the first function)/; s/^/    /' "$n.identical"
    echo "  differing ($(wc -l < "$n.differing")):"; awk -F '\t' '{ print "    " $1 "  (" $2 " lines)" }' "$n.differing"
    echo "  only in old ($(comm -23 "$o.syms" "$n.syms" | wc -l)):"; comm -23 "$o.syms" "$n.syms" | sed 's/^/    /'
    echo "  only in new ($(comm -13 "$o.syms" "$n.syms" | wc -l)):"; comm -13 "$o.syms" "$n.syms" | sed 's/^/    /'
  else
    status=1
    echo "$f: DIFFERS in"
    # every differing line is counted under the function label, kernel descriptor or metadata block it belongs to
    for side in old new; do
      awk '!meta && /^[_A-Za-z][_A-Za-z0-9.$]*:/ { sym = $1 } /^[ \t]*\.amdhsa_kernel / { sym = $2 " (kernel descriptor)" } /^[ \t]*\.amdgpu_metadata/ { meta = 1; sym = "(metadata)" }
           { print sym "\t" $0 }' "$out/$side/${f%.hip}.masked" > "$out/$side/${f%.hip}.bysym"
    done
    diff "$out/old/${f%.hip}.bysym" "$out/new/${f%.hip}.bysym" | sed -n 's/^[<>] \([^\t]*\)\t.*/\1/p' | sort | uniq -c | sed 's/^/   /'
  fi
done
echo "assembly kept in $out"
exit $status
