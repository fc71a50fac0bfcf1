#!/bin/bash
# A/B builds of libnpd.so with every SC unit (npd_sc.hip and the npd_sc_*.hip units that instantiate npd_sc.hpp)
# compiled under experiment macros (tools/bin/libnpd_<name>.so; loaded through NPD_LIB).
# Usage: bash tools/build_sc_variants.sh "name:-DNPD_SC_WPE=3" ...
set -e
cd "$(dirname "$0")/.."
make -j8 lib >/dev/null
mkdir -p tools/bin
units=$(grep -l '#include "npd_sc.hpp"' neural_polar_decoder_amd/csrc/*.hip)
for v in "$@"; do
  n=${v%%:*}; f=${v#*:}
  mkdir -p build/var_$n
  keep=$(ls build/obj/*.o)
  for u in $units; do
    b=$(basename $u .hip)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Iinclude \
      -Ineural_polar_decoder_amd/csrc -munsafe-fp-atomics -fno-honor-nans $f -c $u -o build/var_$n/$b.o &
    keep=$(echo "$keep" | grep -v "/$b.o")
  done
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/bin/libnpd_$n.so $keep build/var_$n/*.o -Wl,--no-undefined
  echo "built tools/bin/libnpd_$n.so ($f)"
done
