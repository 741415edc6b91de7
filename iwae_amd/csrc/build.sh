#!/bin/bash
# Builds libiwae_amd.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -fno-slp-vectorize: packed v_pk_*_f32 next to MFMAs costs more issue slots than it saves (plus v_mov shuffles)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fno-slp-vectorize"
# DIAG=1 ./build.sh: diagnostic library (never the shipped build): the weight-gradient ablation branches (WgradPArgs.dbg), the
# phase-stamp instantiation of out_bwd_pair_kernel and the diagnostic names of iwae_set_option.  STAMPS=1: DIAG plus per-phase
# cycle stamps inside dense_kernel / bern_pipe_kernel / dec_bwd_kernel.
# Build id = sha256 over the sources this library is made of (the same list, order and framing as iwae_amd/_capi.py::source_build_id):
# iwae_build_id() returns it, tests/conftest.py rebuilds when the binary under test does not match the tree, bench.py stamps its line and
# refuses profile artefacts taken on another build.
BUILD_ID=$(for f in activity_kernels.hip aggregate_kernels.hip ais_kernels.hip analysis.hip build.sh device_helpers.h fp32_kernels.hip grid_kernels.hip impute_kernels.hip kernels.h kernels.hip layout.h local_kernels.hip masked_kernels.hip model.h model.hip moments_kernels.hip posterior_kernels.hip row_kernels.hip step_bf16.hip step_f32.hip step_helpers.h update_kernels.hip wgrad_kernels.hip ../../include/iwae_amd.h; do echo "== $(basename $f)"; cat "$f"; done | sha256sum | cut -c1-16)
if [ -n "${DIAG:-}${STAMPS:-}" ]; then BUILD_ID="${BUILD_ID}-diag"; fi
if [ -n "${DIAG:-}${STAMPS:-}" ]; then FLAGS="$FLAGS -DIWAE_DIAG"; fi
if [ -n "${STAMPS:-}" ]; then FLAGS="$FLAGS -DIWAE_DENSE_STAMPS"; fi
# the eighteen translation units compile side by side (fp32_kernels.hip is the long one, kernels.hip the second)
$HIPCC $FLAGS -c kernels.hip -o kernels.o & p1=$!
$HIPCC $FLAGS -DIWAE_BUILD_ID="\"$BUILD_ID\"" -c model.hip -o model.o & p2=$!
$HIPCC $FLAGS -c fp32_kernels.hip -o fp32_kernels.o & p3=$!
$HIPCC $FLAGS -c grid_kernels.hip -o grid_kernels.o & p4=$!
$HIPCC $FLAGS -c activity_kernels.hip -o activity_kernels.o & p5=$!
$HIPCC $FLAGS -c moments_kernels.hip -o moments_kernels.o & p6=$!
$HIPCC $FLAGS -c aggregate_kernels.hip -o aggregate_kernels.o & p7=$!
$HIPCC $FLAGS -c ais_kernels.hip -o ais_kernels.o & p8=$!
$HIPCC $FLAGS -c analysis.hip -o analysis.o & p9=$!
$HIPCC $FLAGS -c local_kernels.hip -o local_kernels.o & p10=$!
$HIPCC $FLAGS -c step_f32.hip -o step_f32.o & p11=$!
$HIPCC $FLAGS -c impute_kernels.hip -o impute_kernels.o & p12=$!
$HIPCC $FLAGS -c posterior_kernels.hip -o posterior_kernels.o & p13=$!
$HIPCC $FLAGS -c row_kernels.hip -o row_kernels.o & p14=$!
$HIPCC $FLAGS -c wgrad_kernels.hip -o wgrad_kernels.o & p15=$!
$HIPCC $FLAGS -c update_kernels.hip -o update_kernels.o & p16=$!
$HIPCC $FLAGS -c masked_kernels.hip -o masked_kernels.o & p17=$!
$HIPCC $FLAGS -c step_bf16.hip -o step_bf16.o & p18=$!
wait $p1; wait $p2; wait $p3; wait $p4; wait $p5; wait $p6; wait $p7; wait $p8; wait $p9; wait $p10; wait $p11; wait $p12; wait $p13; wait $p14; wait $p15; wait $p16; wait $p17; wait $p18
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libiwae_amd.so kernels.o model.o fp32_kernels.o grid_kernels.o activity_kernels.o moments_kernels.o aggregate_kernels.o ais_kernels.o analysis.o local_kernels.o step_f32.o step_bf16.o impute_kernels.o posterior_kernels.o row_kernels.o wgrad_kernels.o update_kernels.o masked_kernels.o -ldl
echo "built $(cd .. && pwd)/libiwae_amd.so (build id $BUILD_ID)"
