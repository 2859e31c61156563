#!/bin/bash
# Build a whole-library variant with extra preprocessor flags (every surfel translation unit, kernels and host side -- msl_sf_*.hip and msl_surfel.hip: all of them see MSL_SUB_ITEMS, MSL_FUSE_CHUNK, MSL_FUSEREC_PLANES): tools/build_full_variant.sh <name> [hipcc flags]
# -> scratch/libmsl_<name>.so (MSL_LIB selects it).  Experiments only.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); NAME=$1; shift
C=$R/manhattanslam_amd/csrc; O=$R/scratch/var_$NAME; mkdir -p $O
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -fno-gpu-flush-denormals-to-zero -I$R/include -I$C"
for o in $(make -s -C $C print-objs | sed 's/\.o//g'); do   # the library's objects, as the Makefile lists them
  case $o in msl_sf_*|msl_surfel) /opt/rocm/bin/hipcc $FLAGS $(make -s -C $C print-file-flags F=$o) "$@" -c $C/$o.hip -o $O/$o.o & ;; *) cp $C/$o.o $O/$o.o ;; esac
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $O/*.o -o $R/scratch/libmsl_$NAME.so
echo built scratch/libmsl_$NAME.so
