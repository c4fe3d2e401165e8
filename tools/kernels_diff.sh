#!/bin/bash
# Are the gfx950 kernels of two builds the same? For every object file named, the device code
# object is taken out of the object file of both build directories (the .hip_fatbin section,
# unbundled) and compared: the symbol list (name, type, size), the disassembly, the .text bytes and
# the metadata notes (per-kernel VGPR / SGPR / scratch / LDS figures). No GPU needed.
#   make -C cpp_raytracer_amd OBJDIR=build_parent OUT=build_parent/lib.so   (in a checkout of the parent)
#   bash tools/kernels_diff.sh <parent build dir> <this build dir> crt_device crt_denoise ...
# Prints one line per comparison, "identical" or "DIFFERS"; exit status 1 when anything differs.
set -o pipefail
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
ARCH=${ARCH:-gfx950}
A=$1; B=$2; shift 2
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
rc=0
for o in "$@"; do
  for side in a b; do
    [ $side = a ] && dir=$A || dir=$B
    out=$tmp/${side}_$o
    $LLVM/llvm-objcopy -O binary --only-section=.hip_fatbin "$dir/$o.o" $out.fatbin || exit 2
    $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --input=$out.fatbin \
      --output=$out.co --unbundle || exit 2
    # addresses left out of the symbol list: only a kernel's name, type and size
    $LLVM/llvm-readelf -sW $out.co | awk 'NR > 3 {print $8, $4, $3}' | sort > $out.syms
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $out.co | grep -v 'file format' > $out.dis
    $LLVM/llvm-objcopy -O binary --only-section=.text $out.co $out.text
    $LLVM/llvm-readelf --notes $out.co > $out.notes
  done
  for ext in syms dis text notes; do
    if cmp -s $tmp/a_$o.$ext $tmp/b_$o.$ext; then
      echo "$o $ext identical ($(wc -c < $tmp/a_$o.$ext) bytes)"
    else
      echo "$o $ext DIFFERS"
      rc=1
    fi
  done
  echo "$o: $(grep -c '\.kd ' $tmp/a_$o.syms) kernels"
done
exit $rc
