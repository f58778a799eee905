cd "${GRAFT_REPO_ROOT:-.}"
O=${OUT:?OUT = folder for the result lines}
mkdir -p $O
for r in 1 2 3; do for n in 2 3; do
  timeout -k 10 300 python bench.py --full --no-beam --no-configs --no-f32-compare --no-cpu-baseline --streams $n > $O/s${n}_$r.json 2> $O/err.txt || exit $?
  echo -n "[$r] streams=$n "; python tools/bench_line.py $O/s${n}_$r.json | cut -c1-40
done; done
