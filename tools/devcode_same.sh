#!/bin/bash
# Is the engine's device code the same bytes as at <git-rev>?  For a change that is meant to leave
# the kernels alone (a move, a host-side fix): no GPU needed, a few minutes on eight cores.
#     tools/devcode_same.sh <git-rev>
# Compiles csrc/cog_engine.hip device-only from an export of <git-rev> and from the working tree,
# each with its own build_ext._compile_cmd flags, for the product build and the three diagnostic
# builds that are kept (COG_TRIO_FENCE, COG_STAMPS, COG_ISSUE_COUNT); prints the sha256 of the
# gfx950 code objects' .text, .rodata and .note side by side; exits non-zero on any difference.
set -euo pipefail
rev=${1:?usage: tools/devcode_same.sh <git-rev>}
root=$(cd "$(dirname "$0")/.." && pwd)
llvm=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
arch=${COG_OFFLOAD_ARCH:-gfx950}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old"
git -C "$root" archive "$rev" | tar -x -C "$tmp/old"

variants="none COG_TRIO_FENCE COG_STAMPS COG_ISSUE_COUNT"
sections=".text .rodata .note"
one() {                                 # tree, tag, variant -> $tmp/tag.variant.<section>
  local def=""
  [ "$3" = none ] || def="-D$3"
  local o="$tmp/$2.$3"
  (cd "$1/gym-eldorado_amd" && python3 -B -c '
import subprocess, sys, build_ext as b
sys.exit(subprocess.call(b._compile_cmd(b.ENGINE_SRCS[0], sys.argv[1], sys.argv[2:]) + ["--cuda-device-only"]))
' "$o.o" $def) > "$o.log" 2>&1 || { cat "$o.log"; return 1; }
  "$llvm/clang-offload-bundler" --unbundle --type=o --targets="hipv4-amdgcn-amd-amdhsa--$arch" \
      --input="$o.o" --output="$o.co"
  for s in $sections; do "$llvm/llvm-objcopy" -O binary --only-section="$s" "$o.co" "$o$s"; done
}
pids=()
for v in $variants; do                  # eight compiles at once
  one "$tmp/old" old "$v" & pids+=($!)
  one "$root" new "$v" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p" || { echo "a compile failed"; exit 2; }; done

rc=0
echo "engine device code ($arch), $(git -C "$root" rev-parse --short "$rev") against the working tree"
for v in $variants; do
  for s in $sections; do
    a=$(sha256sum < "$tmp/old.$v$s" | cut -c1-64)
    b=$(sha256sum < "$tmp/new.$v$s" | cut -c1-64)
    r=same
    [ "$a" = "$b" ] || { r=DIFFERENT; rc=1; }
    printf "%-16s %-8s %9d B  %s  %s  %s\n" "$v" "$s" "$(stat -c %s "$tmp/new.$v$s")" "$a" "$b" "$r"
  done
done
[ $rc = 0 ] && echo "identical" || echo "NOT identical"
exit $rc
