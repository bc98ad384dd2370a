#!/bin/bash
# build_variant.sh NAME "-DFLAG=.. ..." [FAMILY]: libpaoship with one frugal pass-kernel family (csrc/frugal_FAMILY.hip; d4096 =
# the 4096^2 complex128 family by default; d1024, d2048, f2048, f4096) compiled with extra flags -> build/ab/NAME.so (travels to
# the GPU box; build/variants/ does not).  For A/B runs of bench.py on one box (tools/ab_variants.sh selects the variant
# through PAOS_LIB): bench.py repeats to +-0.1 %, tools/fftbench.hip only to +-1.5 %.
set -e
NAME=$1; FLAGS=$2; FAMILY=${3:-d4096}
mkdir -p build/ab
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 -Wall $FLAGS -Ipaos_amd/csrc -c paos_amd/csrc/frugal_$FAMILY.hip -o build/ab/frugal_${FAMILY}_$NAME.o
OBJS=""
for o in build/obj/hip/*.o; do if [ $o = build/obj/hip/frugal_$FAMILY.o ]; then OBJS="$OBJS build/ab/frugal_${FAMILY}_$NAME.o"; else OBJS="$OBJS $o"; fi; done
/opt/rocm/bin/hipcc -shared -fPIC $OBJS build/obj/paos_comm.o build/obj/paos_plan.o build/obj/srchash.o -ldl -o build/ab/$NAME.so
rm -f build/ab/frugal_${FAMILY}_$NAME.o
