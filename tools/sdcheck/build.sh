#!/bin/bash
# Builds tools/sdcheck/sdcheck_bin with the product's host flags (active-orchard-slam_amd/Makefile).
# build.sh poison: tools/sdcheck/sdcheck_bin_poison with -DAOS_SD_POISON (pending fields hold INT_MIN, subdiv2d.h).
# build.sh asan:   tools/sdcheck/sdcheck_bin_asan, the poison build under AddressSanitizer and UBSan (host only;
#                  run it with AOS_SDCHECK_REPS=4 or so).
set -e
D=$(cd "$(dirname "$0")" && pwd)
case "$1" in
  poison) X="-O3 -DAOS_SD_POISON"; OUT=sdcheck_bin_poison ;;
  asan)   X="-O1 -g -DAOS_SD_POISON -fsanitize=address,undefined -fno-sanitize-recover=undefined"; OUT=sdcheck_bin_asan ;;
  *)      X="-O3"; OUT=sdcheck_bin ;;
esac
/opt/rocm/bin/hipcc -x c++ $X -std=c++17 -ffp-contract=off -fno-fast-math -march=x86-64-v3 -mtune=znver5 -I"$D/../../active-orchard-slam_amd/csrc" \
  "$D/sdcheck.cpp" "$D/../../active-orchard-slam_amd/csrc/subdiv2d.cpp" -o "$D/$OUT"
