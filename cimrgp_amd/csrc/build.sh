#!/bin/bash
# Build libcimrgp.so for gfx950 (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
OBJS=()
pids=()
for f in api block gemm_nt potrf gram solve misc reduced layer comm joint grad loo svgp psi psi_grad psi_rows inducing sparse sparse_post sparse_grad; do
    stale=0
    if [ ! -f "$f.o" ] || [ "$f.hip" -nt "$f.o" ]; then stale=1; fi
    for h in *.hpp ../../include/*.h; do
        if [ "$h" -nt "$f.o" ]; then stale=1; fi
    done
    if [ $stale = 1 ]; then
        $HIPCC $FLAGS -c "$f.hip" -o "$f.o" &
        pids+=($!)
    fi
    OBJS+=("$f.o")
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libcimrgp.so "${OBJS[@]}" -ldl
echo "built $(cd .. && pwd)/libcimrgp.so"
