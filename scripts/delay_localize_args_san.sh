#!/bin/bash
# Host AddressSanitizer + UndefinedBehaviorSanitizer over the host side of
# acl_fleet_delay_localize_batch (the argument checks and the workspace size in
# csrc/fleet_localize.hip), as a stand-alone program
# (tests/delay_localize_args_san_main.cpp). Needs no GPU: every call fails a
# check before any HIP call. The device code is compiled as usual and never
# launched. Run: bash scripts/delay_localize_args_san.sh  (writes build/san/)
set -o pipefail
cd "$(dirname "$0")/.."
O=build/san
mkdir -p $O
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-omit-frame-pointer \
    -Xarch_host -fsanitize=address,undefined -Wall -Wno-unused-function -Iinclude \
    aclswarm_amd/csrc/fleet_localize.hip -x hip tests/delay_localize_args_san_main.cpp \
    -o $O/delay_localize_args_san || exit 1
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
    timeout -k 10 120 $O/delay_localize_args_san 2>&1 | tee $O/delay_localize_args_san.txt | tail -20
