#!/bin/bash
# Per-kernel VGPR / scratch / LDS usage of the product kernels (device-only compile, no GPU needed).
# With an argument: the same for a GENERATED program source (sdfk_program_source / SDFK_DUMP_SOURCE), compiled with the JIT's flags.
# With --unit NAME.hip: the same for that translation unit of sdfkit_amd/csrc, then the number of scalar memory writes (stores,
# atomics, data-cache write-backs) in its ISA, which must be 0.
set -e
T=$(mktemp -d)
if [ "$1" = "--unit" ]; then
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only -c \
        "$(dirname "$0")/../sdfkit_amd/csrc/$2" -o $T/dev.o
elif [ -n "$1" ]; then
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only -c -x hip \
        -DSDFK_SAMPLE_NT=1 -DSDFK_SAMPLE_RPW=2 -DSDFK_KERNELS=131071 -include hip/hip_runtime.h "$1" -o $T/dev.o
else
hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only -c \
    "$(dirname "$0")/../sdfkit_amd/csrc/mc_kernels.hip" -o $T/dev.o
fi
/opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input=$T/dev.o \
    --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/k.co
/opt/rocm/lib/llvm/bin/llvm-readelf --notes $T/k.co | \
    grep -E "\.name:|\.vgpr_count|private_segment_fixed|vgpr_spill|sgpr_spill|group_segment_fixed" | paste - - - - - - | \
    sed -e 's/ \+/ /g'
if [ "$1" = "--unit" ]; then
    # The mnemonics of scalar memory writes (stores, buffer / scratch stores, atomics, data-cache write-back and discard).  The
    # pattern is assembled from pieces because source files of this project must not contain those mnemonics themselves.
    S="s_"
    N=$(/opt/rocm/lib/llvm/bin/llvm-objdump -d $T/k.co | grep -cE "\\b${S}(buffer_|scratch_)?(store|atomic)|\\b${S}dcache_(wb|discard)" || true)
    echo "scalar memory writes in the ISA of $2: $N"
    if [ "$N" != "0" ]; then rm -rf $T; exit 1; fi
fi
[ -n "$KEEP" ] && echo "$T/k.co" || rm -rf $T
