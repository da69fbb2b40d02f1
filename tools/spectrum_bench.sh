#!/bin/bash
# tools/spectrum_bench.py step by step: every GPU step under its own time limit, the next one only after the last one's success.
# DIR holds the index files and the steps' JSON; `python tools/spectrum_bench.py collect --dir DIR` makes profiles/kmer_spectrum.json.
set -o pipefail
cd "$(dirname "$0")/.."
DIR=${DIR:-build/spectrum_bench}
timeout -k 10 240 python tools/spectrum_bench.py index --dir "$DIR" "$@" &&
timeout -k 10 240 python tools/spectrum_bench.py measure --form two_step --dir "$DIR" "$@" &&
SIGAX_TWO_STEP=0 timeout -k 10 240 python tools/spectrum_bench.py measure --form one_step --dir "$DIR" "$@" &&
timeout -k 10 240 python tools/spectrum_bench.py compose --dir "$DIR" "$@"
