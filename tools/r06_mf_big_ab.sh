#!/bin/bash
# Which fronts take the row-block solve (EIGSOL_MF_BIG_NS pivots; shipped 96, or 256 rows), after the
# premultiplied blocks, 1M convection-diffusion (tools/mf_probe.py), two rounds
set -o pipefail
mkdir -p gpurun_out/r6
O=gpurun_out/r6/mf_big_ab.log
: > $O
for r in 1 2; do
  for ns in 96 64 128 192; do
    echo "EIGSOL_MF_BIG_NS=$ns" >> $O
    EIGSOL_MF_BIG_NS=$ns timeout -k 10 200 python -u tools/mf_probe.py 1000 >> $O 2>&1 || exit 1
  done
done
cat $O
