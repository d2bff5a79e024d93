#!/bin/bash
# Host AddressSanitizer + UndefinedBehaviorSanitizer over the host side of
# acl_fleet_delay_est_trial_init / acl_fleet_delay_est_trial_batch (the argument
# checks in csrc/fleet_trial.hip), as a stand-alone program
# (tests/delay_est_trial_args_san_main.cpp). Needs no GPU: every call fails a
# check before any HIP call. fleet_trial.hip's host code is compiled with the
# sanitizers; the entries it would call come from the built library
# (python -m aclswarm_amd.build first) and are never reached. The device code is
# compiled as usual and never launched.
# Run: bash scripts/delay_est_trial_args_san.sh  (writes build/san/)
set -o pipefail
cd "$(dirname "$0")/.."
O=build/san
mkdir -p $O
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-omit-frame-pointer \
    -Xarch_host -fsanitize=address,undefined -Wall -Wno-unused-function -Iinclude \
    aclswarm_amd/csrc/fleet_trial.hip -x hip tests/delay_est_trial_args_san_main.cpp \
    -Laclswarm_amd/lib -laclswarm_amd -Wl,-rpath,"$PWD/aclswarm_amd/lib" \
    -o $O/delay_est_trial_args_san || exit 1
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
    timeout -k 10 120 $O/delay_est_trial_args_san 2>&1 | tee $O/delay_est_trial_args_san.txt | tail -20
