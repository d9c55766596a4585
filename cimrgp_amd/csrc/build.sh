#!/bin/bash
# Build libcimrgp.so for gfx950 (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
OBJS=()
pids=()
for f in api block gemm_nt potrf gram solve misc reduced layer comm joint grad loo sparse sparse_post sparse_grad; do
    if [ ! -f "$f.o" ] || [ "$f.hip" -nt "$f.o" ] || [ common.hpp -nt "$f.o" ] || [ abi.hpp -nt "$f.o" ] || [ gemm_tile.hpp -nt "$f.o" ] || [ chain_kernels.hpp -nt "$f.o" ] || [ rows_kernels.hpp -nt "$f.o" ] || [ ../../include/cimrgp.h -nt "$f.o" ] || [ ../../include/cimrgp_objective.h -nt "$f.o" ] || [ ../../include/cimrgp_joint.h -nt "$f.o" ] || [ ../../include/cimrgp_grad.h -nt "$f.o" ] || [ ../../include/cimrgp_loo.h -nt "$f.o" ] || [ ../../include/cimrgp_sparse.h -nt "$f.o" ] || [ ../../include/cimrgp_sparse_grad.h -nt "$f.o" ] || [ ../../include/cimrgp_sparse_layer.h -nt "$f.o" ] || [ ../../include/cimrgp_sparse_ard.h -nt "$f.o" ] || [ ../../include/cimrgp_layer_ard.h -nt "$f.o" ] || [ ../../include/cimrgp_sparse_post.h -nt "$f.o" ]; then
        $HIPCC $FLAGS -c "$f.hip" -o "$f.o" &
        pids+=($!)
    fi
    OBJS+=("$f.o")
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libcimrgp.so "${OBJS[@]}" -ldl
echo "built $(cd .. && pwd)/libcimrgp.so"
