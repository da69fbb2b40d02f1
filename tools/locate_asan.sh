#!/bin/bash
# sigah::Locator's batching and formatting under AddressSanitizer + UBSan, without a GPU and without a Python in between:
# tools/locate_asan_driver.cpp is a program of its own that compiles siga_amd/host/locate.cpp and reads.cpp with a stub in
# place of the library (no runtime is preloaded into anything).
#   bash tools/locate_asan.sh
set -eu
cd "$(dirname "$0")/.."
mkdir -p build
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-sign-compare \
    -o build/locate_asan_driver tools/locate_asan_driver.cpp siga_amd/host/locate.cpp siga_amd/host/reads.cpp -lz
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
ASAN_OPTIONS=detect_leaks=1 timeout -k 10 600 build/locate_asan_driver "$D"
