#!/bin/bash
# Host-side AddressSanitizer run (no GPU: CPU mode only) of the cross-capacity
# checkpoint save / load and mbots_max_population (tests/c_host/cap_asan.c) and
# of the capacity growth in place with its retired lists
# (tests/c_host/grow_asan.c, also under UndefinedBehaviorSanitizer) and of the
# episode entry points (tests/c_host/reset_host.c, likewise) and of the trajectory
# window (tests/c_host/traj_host.c, likewise) through the C ABI, against a libmbots built with -Xarch_host -fsanitize=address,undefined
# (the device code is not instrumented).  Where the reference's simulation
# source lies on the machine (REF, default /root/reference), also a short
# lock-step of the oracle with that source on the stand-in engine
# (tests/c_host/ref_lockstep_asan.cpp; oracle/Makefile), all of it under both
# sanitizers: the reference's read of rewards[4] must stay inside
# the stand-in's own storage.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
d=$(mktemp -d)
(cd $ROOT/madrona-bots_amd/csrc && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC \
    -ffp-contract=off -fno-slp-vectorize -Xarch_host -fsanitize=address,undefined -shared -o $d/libmbots_asan.so \
    mbots_kernels.hip mbots_manager.cpp mbots_cpu.cpp)
/opt/rocm/llvm/bin/clang -g -fsanitize=address -std=c99 -I$ROOT/include $ROOT/tests/c_host/cap_asan.c \
    -L$d -lmbots_asan -Wl,-rpath,$d -o $d/cap_asan
ASAN_OPTIONS=detect_leaks=0 $d/cap_asan
/opt/rocm/llvm/bin/clang -g -fsanitize=address,undefined -std=c99 -I$ROOT/include $ROOT/tests/c_host/grow_asan.c \
    -L$d -lmbots_asan -Wl,-rpath,$d -o $d/grow_asan
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $d/grow_asan
/opt/rocm/llvm/bin/clang -g -fsanitize=address,undefined -std=c99 -I$ROOT/include $ROOT/tests/c_host/reset_host.c \
    -L$d -lmbots_asan -Wl,-rpath,$d -o $d/reset_host
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $d/reset_host
/opt/rocm/llvm/bin/clang -g -fsanitize=address,undefined -std=c99 -I$ROOT/include $ROOT/tests/c_host/traj_host.c \
    -L$d -lmbots_asan -Wl,-rpath,$d -o $d/traj_host
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $d/traj_host
REF=${REF:-/root/reference}
if [ -f $REF/src/sim/sim.cpp ]; then
    make -s -C $ROOT/oracle REF=$REF REF_OUT=$d/ref \
        REF_EXTRA="-g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined" \
        $d/ref/ref_lockstep_asan
    ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $d/ref/ref_lockstep_asan
else
    echo "asan_host: no reference source at $REF: ref_lockstep_asan not run"
fi
rm -rf $d
