set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-out}/g49; mkdir -p $O
for k in 0 1 0 1; do
  HIP_FORCE_DEV_KERNARG=$k timeout -k 10 200 python -u bench.py --full --no-cpu-baseline > $O/b_$k.json 2> $O/b_$k.err || exit $?
  python3 -c "import json;d=json.loads(open('$O/b_$k.json').read().strip().splitlines()[-1]);print('kernarg=$k', d['value'], d['roofline']['avg_launch_ms'], d['ms_per_step'], d['sorted_result']['value'])"
done
