# A/B bench on one box (development tool): A = yolo-continuous_amd/ycx/libycx_A.so, B = the in-tree library.
# Run from the repository root; logs go to $YCX_OUT (default: out/).
R=$(cd "$(dirname "$0")/.." && pwd)
A=$R/yolo-continuous_amd/ycx/libycx_A.so
O=${YCX_OUT:-$R/out}
mkdir -p "$O"
for v in A B A B; do
  if [ $v = A ]; then export YCX_LIB=$A; else unset YCX_LIB; fi
  timeout -k 10 200 python bench.py --full --cpu-seconds 0 > "$O/ab_$v.log" 2>&1 || exit 1
  tail -1 "$O/ab_$v.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v', d['value'], d['ms_per_step'], d['p50_ms'], d['roofline']['forward_kernel_ms'])"
done
