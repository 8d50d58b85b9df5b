#!/bin/bash
# Host-side AddressSanitizer run (no GPU: CPU mode only) of the cross-capacity
# checkpoint save / load and mbots_max_population (tests/c_host/cap_asan.c) and
# of the capacity growth in place with its retired lists
# (tests/c_host/grow_asan.c, also under UndefinedBehaviorSanitizer) and of the
# episode entry points (tests/c_host/reset_host.c, likewise) and of the trajectory
# window (tests/c_host/traj_host.c, likewise) through the C ABI, against a libmbots built with -Xarch_host -fsanitize=address,undefined
# (the device code is not instrumented).
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
rm -rf $d
