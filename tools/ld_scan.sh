#!/bin/bash
# Lab script: the real reduction at N=8192 on caller buffers with different leading dimensions.  Separate processes,
# two rounds.
cd "$(dirname "$0")/.."
for i in 1 2; do
  for lda in 8224 8256 8288 8320 8352 8448 8704 9216; do
    echo -n "reduce lda $lda: "
    EIGX_MF=64 EIGX_LDA=$lda timeout -k 10 200 python tools/gpu_reduce_time.py 8192 2 2 2>&1 | grep "rep [12]" | sed -e "s/(.*//" | tr "\n" " "
    echo
  done
done
