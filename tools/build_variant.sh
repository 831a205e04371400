#!/bin/bash
# A/B builds of the development library (BLS12-381 G1 + Fr only; other curves return ARK_HIP_ERR_ARG):
#   tools/build_variant.sh NAME [extra hipcc flags, e.g. -DARK_LAZY_MIN_WAVES=1]
# -> algebra_amd/variants/libark_hip_NAME.so; select it with ARK_HIP_LIB=<path> (algebra_amd/_lib.py)
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
S=$R/algebra_amd/csrc
O=/tmp/ark_variant_$name
mkdir -p $O $R/algebra_amd/variants
FL="-O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-result -Wno-pass-failed -I$S $*"
CAPI="runtime msm fft poly comm points"   # CAPI_OBJS of csrc/Makefile
pids=()
for u in $CAPI; do /opt/rocm/bin/hipcc $FL -DARK_HIP_DEV -c $S/capi_$u.hip -o $O/capi_$u.o & pids+=($!); done
/opt/rocm/bin/hipcc $FL -DARK_UNIT_CURVE=BLS12_381_G1 -c $S/curve_unit.hip -o $O/msm.o & pids+=($!)
/opt/rocm/bin/hipcc $FL -DARK_UNIT_FIELD=BLS12_381_FR -c $S/field_unit.hip -o $O/fft.o & pids+=($!)
for p in "${pids[@]}"; do wait $p; done   # a failed compile stops the build (set -e)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/algebra_amd/variants/libark_hip_$name.so \
  $(for u in $CAPI; do echo $O/capi_$u.o; done) $O/msm.o $O/fft.o
echo built $R/algebra_amd/variants/libark_hip_$name.so
