export TMPDIR=/tmp
REPO=${GRAFT_REPO_ROOT:-$PWD}; OUT=$REPO/gpurun_out; tag=r06f
cd $REPO
timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err && echo rc=0 || { echo "bench rc=$?"; exit 1; }
rm -rf $OUT/prof/${tag}_bench
( cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof/${tag}_bench -o bench -- python $REPO/bench.py --steps 3 --warmup 1 --no-cpu-baseline --full > $OUT/${tag}_bench_under_rocprof.json 2> $OUT/${tag}_bench_under_rocprof.err ) || exit 1
find $OUT/prof/${tag}_bench -name "*kernel_stats.csv" -exec cp {} $OUT/${tag}_bench_kernel_stats.csv \;
