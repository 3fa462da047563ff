set -e
O=${OUT:?set OUT to the output directory}/c4
mkdir -p $O
for b in 1024 512 256 128; do
  timeout -k 10 120 python bench.py --full --workload c4 --batch $b --no-cpu-baseline > $O/b$b.json 2>$O/b$b.err
  timeout -k 10 120 python bench.py --workload c4 --batch $b > $O/b${b}_graph.json 2>>$O/b$b.err
done
export TMPDIR=/tmp
timeout -k 10 180 rocprofv3 --kernel-trace --stats -d $O/prof128 -o run --output-format csv -- python bench.py --full --workload c4 --batch 128 --no-cpu-baseline --steps 5 --warmup 1 > $O/prof128.log 2>&1
echo done
