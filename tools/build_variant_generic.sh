#!/bin/bash
# Diagnostic build with extra -D flags on the layer-wise path's two units, objnerf_generic.hip (network, small-batch
# kernels) and objnerf_gemm.hip (the GEMM layer: OBJ_GEMM_BK and the other tile sizes live there):
#   tools/build_variant_generic.sh NAME -DOBJ_GEMM_BK=32
set -e
cd "$(dirname "$0")/../openobj_amd/csrc"
name=$1; shift
mkdir -p abl
make -s
for u in generic gemm; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off "$@" -c objnerf_$u.hip -o abl/${u}_$name.o
done
others=$(ls objnerf_*.o | grep -v -e '^objnerf_generic\.o$' -e '^objnerf_gemm\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o abl/lib_$name.so $others abl/generic_$name.o abl/gemm_$name.o
echo built abl/lib_$name.so
