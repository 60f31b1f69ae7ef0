#!/bin/bash
# One profiler run of the headline step with the per-robot broadphase compiled under extra options (nbk_bf32_spec.hpp's switches).
# usage (from the repository root, on a machine with the GPU): bash tools/spec_variant.sh <tag> trace|pmc [<library>|-] ["<NBK_JIT_OPTIONS>"] [bench args...]
#   trace: rocprofv3 --kernel-trace --stats over bench.py --steps 20 --warmup 3  -> <out>/<tag>_bench_kernel_stats.csv
#   pmc:   rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES (a run of its own, no tracing) over --steps 3 --warmup 1
#          -> <out>/<tag>_pmc_sq_counter_collection.csv      (<out>: $SPEC_VARIANT_OUT, default profiles)
# <library>: another build of libnbk.so (numbotics_amd._lib.LIB_PATH is pointed at it before bench.py runs), - for this tree's.  Prints one line (tools/spec_variant.py).
# The DIAG switches give wrong masks on purpose: bench.py's parity line then says so; the kernel times and counters are what is read.
set -o pipefail
O=${SPEC_VARIANT_OUT:-profiles}
tag=$1; mode=$2; lib=${3:--}; opts=${4:-}; shift; shift; shift; shift
export TMPDIR=/tmp
[ -n "$opts" ] && export NBK_JIT_OPTIONS="$opts"
run=(python3 bench.py)
[ "$lib" != "-" ] && run=(python3 -c "import os, runpy, sys; sys.path.insert(0, os.getcwd()); from numbotics_amd import _lib; _lib.LIB_PATH = os.path.abspath(sys.argv[1]); sys.argv = ['bench.py'] + sys.argv[2:]; runpy.run_path('bench.py', run_name='__main__')" "$lib")
out=$O/${tag}_${mode}
mkdir -p "$O"
if [ "$mode" = trace ]; then
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out" -- "${run[@]}" --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --no-extras "$@" > "$out.log" 2>&1 < /dev/null
    rc=$?
    f=$(find "$out" -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] && cp "$f" "$O/${tag}_bench_kernel_stats.csv"
else
    timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv -d "$out" -- "${run[@]}" --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-extras "$@" > "$out.log" 2>&1 < /dev/null
    rc=$?
    f=$(find "$out" -name '*counter_collection.csv' | head -1)
    [ -n "$f" ] && cp "$f" "$O/${tag}_pmc_sq_counter_collection.csv"
fi
[ -n "$f" ] && python3 tools/spec_variant.py "$tag" "$mode" "$f" "$out.log" "$opts"
rm -rf "$out"
exit $rc
