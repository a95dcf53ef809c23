#!/bin/bash
# CPU sanitizer run: the host side of libfa2_hip.so and the oracle, built with AddressSanitizer + UBSan, under
# the CPU tests that exercise them -- argument validation and the tile table through the C ABI (tests/test_abi.py), the oracle
# against the golden vectors (tests/test_oracle.py).  GPU sanitizers are not available on the pool: this is the CPU build only.
# The library's tile query asks the HIP runtime for the device; with a GPU present that brings the device up inside the sanitized
# process, which aborts.  So this runs only where there is no GPU.
set -eu
if [ -e /dev/kfd ]; then echo "run_asan.sh: a host-side sanitizer run, for a machine without a GPU (/dev/kfd is present)" >&2; exit 3; fi
cd "$(dirname "$0")/.."
LOG=$(mktemp)
trap 'rm -f "$LOG"' EXIT
make -C flash_attention_dlrs_amd/csrc asan -j8 > "$LOG" 2>&1 || { tail -20 "$LOG"; exit 2; }
make -C oracle asan > /dev/null
RT=$(ls /opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so | head -1)
# the sanitizer run time goes first; whatever the environment already preloads stays after it
export LD_PRELOAD="$RT${LD_PRELOAD:+ $LD_PRELOAD}" ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1
export FA2_HIP_LIB=$PWD/flash_attention_dlrs_amd/libfa2_hip_asan.so FA2_ORACLE_LIB=$PWD/oracle/libfa2_oracle_asan.so
"${PYTHON:-python3}" -m pytest tests/test_abi.py tests/test_oracle.py tests/test_oracle_bwd.py -q -m "not gpu" -p no:cacheprovider "$@"
