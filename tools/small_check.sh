set -e
O=${OUT:?set OUT to the output directory}
mkdir -p $O/c4
timeout -k 10 120 ipm-zoo_amd/build/kbench 320 small > $O/kb_small.log 2>&1
timeout -k 10 300 python -u -m pytest tests/test_gpu_batch.py -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $O/c4/tests.log 2>&1
for b in 1024 128; do
  timeout -k 10 120 python bench.py --full --workload c4 --batch $b --no-cpu-baseline > $O/c4/b$b.json 2>$O/c4/b$b.err
done
