#!/bin/sh
# codehash.sh ARCH obj...: for each device-only object (hipcc --cuda-device-only -c) print
#   TU  sha256(.text)  sha256(.rodata)  sha256(kernel descriptors)
# of its ARCH code object.
#   .text        the machine code: equal = the same instructions in the same order.
#   .rodata      the section holding the kernel descriptors (register counts, LDS, scratch),
#                bytes as they are: equal = the same kernels with the same resources at the
#                same addresses.  It changes when a kernel is renamed: a shorter or longer
#                mangled name moves the sections in front of .rodata, and each descriptor
#                stores its code's entry as an offset from its own address.
#   descriptors  the 64 bytes at every symbol ending in .kd, in address order, with bytes
#                16-23 (that code-entry offset) zeroed: equal = the same kernels in the same
#                order with the same resources, whatever they are called.
# The other sections carry names and a per-compilation id that changes with any edit of the
# source, so the whole file is not compared.  Called by `make codehash` in
# mcmc-for-nested-data_amd/csrc.
set -e
LLVM=${LLVM:-/opt/rocm/llvm/bin}
arch=$1; shift
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for o in "$@"; do
  tu=$(basename "$o" .o)
  if ! "$LLVM/clang-offload-bundler" --unbundle --type=o --input="$o" --output="$tmp/$tu.elf" \
       --targets=hip-amdgcn-amd-amdhsa--$arch 2>/dev/null || [ ! -s "$tmp/$tu.elf" ]; then
    cp "$o" "$tmp/$tu.elf"   # already a bare code object
  fi
  for sec in text rodata; do
    : > "$tmp/$tu.$sec"
    "$LLVM/llvm-objcopy" -O binary --only-section=.$sec "$tmp/$tu.elf" "$tmp/$tu.$sec"
  done
  # the descriptors: .rodata's address, then every .kd symbol's offset into it
  ro=$("$LLVM/llvm-readelf" -S -W "$tmp/$tu.elf" | sed 's/^ *\[ *[0-9]*\] *//' |
       awk '$1 == ".rodata" { print $3 }')
  : > "$tmp/$tu.kd"
  "$LLVM/llvm-readelf" -s -W "$tmp/$tu.elf" | awk '$8 ~ /\.kd$/ { print $2 }' | sort -u |
  while read -r addr; do
    off=$((0x$addr - 0x$ro))
    dd if="$tmp/$tu.rodata" bs=1 skip=$off count=16 2>/dev/null
    head -c 8 /dev/zero
    dd if="$tmp/$tu.rodata" bs=1 skip=$((off + 24)) count=40 2>/dev/null
  done >> "$tmp/$tu.kd"
  printf '%-18s %s  %s  %s\n' "$tu" "$(sha256sum < "$tmp/$tu.text" | cut -d' ' -f1)" \
                                    "$(sha256sum < "$tmp/$tu.rodata" | cut -d' ' -f1)" \
                                    "$(sha256sum < "$tmp/$tu.kd" | cut -d' ' -f1)"
done
