# The whole check on a GPU machine: GPU suite, smoke, the full bench, the one-rank RCCL rehearsal.
# Logs go to $YCX_OUT (default: out/final under the repository root).
R=$(cd "$(dirname "$0")/.." && pwd)
O=${YCX_OUT:-$R/out/final}
mkdir -p "$O"
cd "$R"
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$O/gputests.log" 2>&1 || { tail -40 "$O/gputests.log"; exit 1; }
tail -2 "$O/gputests.log"
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || { tail -20 "$O/smoke.log"; exit 1; }
tail -1 "$O/smoke.log"
timeout -k 10 300 python bench.py --full > "$O/bench.log" 2>&1 || { tail -20 "$O/bench.log"; exit 1; }
tail -1 "$O/bench.log" | cut -c1-400
timeout -k 10 300 python bench.py --full --dist --cpu-seconds 0 >"$O/dist.log" 2>&1 || { tail -20 "$O/dist.log"; exit 1; }
tail -1 "$O/dist.log" | cut -c1-300
