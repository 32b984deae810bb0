#!/usr/bin/env bash
# Build liblpi_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable"
mkdir -p build
pids=()
for f in api gemm gemm256 gemm256p gemm256x128 gemm_rows gemm_mx8 mx8_rows mx4_rows attention attention4 attn_pooled attn_stream attn_long attn_hd attn_hd88 attn_hd104 rowops posembed act loss interact bpe host imageops jpeg search search16 search_mx8 search_mx4 search_wide search_rerank; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ common.h -nt build/$f.o ] || [ dispatch.h -nt build/$f.o ] || [ gemm_host.h -nt build/$f.o ] || [ gemm_epilogue.h -nt build/$f.o ] || [ attn_softmax.h -nt build/$f.o ] || [ attn_walk.h -nt build/$f.o ] || [ attn_hd_widths.h -nt build/$f.o ] || [ unicode_ln.h -nt build/$f.o ] || [ gemm256_tile.h -nt build/$f.o ] || [ gemm256x128_tile.h -nt build/$f.o ] || [ mx8.h -nt build/$f.o ] || [ mx4.h -nt build/$f.o ] || [ search_tile.h -nt build/$f.o ] || [ ../../include/lpi_hip.h -nt build/$f.o ]; then
    extra=""
    case $f in attention|attention4) extra="-fno-honor-nans";; esac      # see attn_softmax.h (attn_max3)
    $HIPCC $FLAGS $extra -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o liblpi_hip.so build/api.o build/gemm.o build/gemm256.o build/gemm256p.o build/gemm256x128.o build/gemm_rows.o build/gemm_mx8.o build/mx8_rows.o build/mx4_rows.o build/attention.o build/attention4.o build/attn_pooled.o build/attn_stream.o build/attn_long.o build/attn_hd.o build/attn_hd88.o build/attn_hd104.o build/rowops.o build/posembed.o build/act.o build/loss.o build/interact.o build/bpe.o build/host.o build/imageops.o build/jpeg.o build/search.o build/search16.o build/search_mx8.o build/search_mx4.o build/search_wide.o build/search_rerank.o -lpthread
echo "built $(pwd)/liblpi_hip.so"
