# A/B of two builds of the library on one box: default, then $ALT (copied over the default);
# the result lines go to $OUT
cd $GRAFT_REPO_ROOT
O=${OUT:?OUT = folder for the result lines}
mkdir -p $O
run() {
  timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-f32-compare > $O/ab_$1.json 2> $O/ab_$1.err || { tail -5 $O/ab_$1.err; exit 1; }
  python -c "import json; d=json.load(open('$O/ab_$1.json')); print('$1', round(d['ms_per_step'],3), round(d['beam']['ms_per_step'],3), d['kernel_breakdown_ms'])"
}
run base
cp chinese-asr_amd/casr/libcasr_hip.so /tmp/base.so
cp chinese-asr_amd/casr/$ALT chinese-asr_amd/casr/libcasr_hip.so
run alt
cp /tmp/base.so chinese-asr_amd/casr/libcasr_hip.so
run base2
