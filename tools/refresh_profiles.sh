set -e
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
O=build/ref
mkdir -p $O
timeout -k 5 200 python bench.py --full > $O/bench.json 2> $O/bench.err
echo bench done
timeout -k 5 200 rocprofv3 --kernel-trace --stats --output-format csv -d $O/ks -- python3 bench.py --steps 100 --warmup 10 --cpu-seconds 0 --no-split > $O/ks.log 2>&1
echo stats done
KM_BENCH_NO_SPINUP=1 timeout -k 5 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/fetch -- python3 bench.py --steps 20 --warmup 5 --cpu-seconds 0 --no-split > $O/fetch.log 2>&1
echo fetch done
KM_BENCH_NO_SPINUP=1 timeout -k 5 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/write -- python3 bench.py --steps 20 --warmup 5 --cpu-seconds 0 --no-split > $O/write.log 2>&1
echo write done
