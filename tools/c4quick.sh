# C4 quick check: batch tests, then the batch sweep (default and IPMZ_DIAG=blk)
set -e
O=${OUT:?set OUT to the output directory}/c4
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_batch.py -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $O/tests.log 2>&1
for b in 1024 128; do
  timeout -k 10 120 python bench.py --full --workload c4 --batch $b --no-cpu-baseline > $O/b$b.json 2>$O/b$b.err
  IPMZ_SMALL=0 timeout -k 10 120 python bench.py --full --workload c4 --batch $b --no-cpu-baseline > $O/b${b}_old.json 2>>$O/b$b.err
done
echo done
