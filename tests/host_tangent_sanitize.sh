#!/bin/bash
# CPU only: tests/host_tangent_harness.cpp (the pool, the expanders and the chunk plan of csrc/fcamd_hosttangent.cpp behind stubs of
# the HIP calls) built with ThreadSanitizer and with AddressSanitizer + UBSan, every case of tests/test_host_tangent_pool.py through both.
# Sanitizers run on this host code only, never on the GPU.
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
exec python3 -m pytest -x -q -p no:cacheprovider -m "not gpu" tests/test_host_tangent_pool.py -k "tsan or asan_ubsan" "$@"
