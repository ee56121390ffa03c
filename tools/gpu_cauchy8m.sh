# Cauchy-good encode at C = 4 MiB vs 8 MiB (same bytes per launch): kernel time, L2 and UTCL1
# counters, one rocprofv3 --pmc pass per counter group.  VERDICT r01 "what's weak" 5.
set -o pipefail
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out/c8m; export TMPDIR=/tmp
A="TCP_UTCL1_TRANSLATION_MISS_sum TCP_UTCL1_TRANSLATION_HIT_sum TCP_UTCL1_STALL_MULTI_MISS_sum TCP_UTCL1_THRASHING_STALL_sum"
B="TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum"
for cfg in "20 6 4194304 102" "20 6 8388608 51" "10 4 4194304 204" "10 4 8388608 102"; do
  set -- $cfg
  tag="k$1m$2c$(( $3 >> 20 ))"
  B0="python $PWD/bench.py --full --method cauchy_good --k $1 --m $2 --chunk $3 --stripes $4 --steps 3 --warmup 1 --no-cpu --no-host-path --no-layout-ab --no-copy-ref"
  timeout -k 10 120 $B0 --json-out gpurun_out/c8m/bench_$tag.json > gpurun_out/c8m/bench_$tag.log 2>&1 || exit 1
  timeout -s KILL 90 rocprofv3 --pmc $A --kernel-trace --output-format csv -d gpurun_out/c8m/utcl_$tag -o p -- $B0 > gpurun_out/c8m/utcl_$tag.log 2>&1 || exit 1
  timeout -s KILL 90 rocprofv3 --pmc $B --output-format csv -d gpurun_out/c8m/tcc_$tag -o p -- $B0 > gpurun_out/c8m/tcc_$tag.log 2>&1 || exit 1
  echo "ok $tag"
done
