#!/bin/bash
# The HOST side of the mirror chain (csrc/rt_mirror.hip: the argument checks and the chunk arithmetic, everything that needs
# no device) under AddressSanitizer, as a stand-alone program with its own main (scripts/asan_mirror_host.hip), on a machine
# without a GPU.  rt_capi.hip, which owns the handle and the rules the checks call, is compiled with the sanitizer as well; the
# device code and the other units are the product build's objects.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:-/tmp/tcrt_asan_mirror}
mkdir -p $O
cd $R/tilecoderaytracer_amd/csrc
make -j8 >/dev/null
HF="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -fno-fast-math -fno-slp-vectorize"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer"
/opt/rocm/bin/hipcc $HF $SAN -c rt_capi.hip -o $O/rt_capi.o
/opt/rocm/bin/hipcc $HF $SAN -c $R/scripts/asan_mirror_host.hip -o $O/asan_mirror_host.o
OTHERS=$(ls *.o | grep -v -e '^rt_capi.o$' -e '^rt_mirror.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address -o $O/asan_mirror_host $O/asan_mirror_host.o $O/rt_capi.o $OTHERS -ldl
ASAN_OPTIONS=detect_leaks=0 $O/asan_mirror_host
