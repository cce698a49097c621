# GEMV kernels with HBM-cold weights (rotated copies) and with one hot copy (<= 256 MB products then sit in the Infinity Cache)
#   bash tools/kb_gemv.sh [gemv|gemv8|gemv4]      the kbench.py case: bf16, e4m3 or MXFP4 weights (the format is the kernel's first template argument)
# KB_OUT: where the two kbench logs are kept (default: a fresh temporary directory, named at the end); the traces are removed
set -e
CASE=${1:-gemv}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${KB_OUT:-$(mktemp -d)}
mkdir -p $OUT
for mode in cold hot; do
  rm -rf $OUT/kbv_$mode && mkdir -p $OUT/kbv_$mode
  if [ $mode = hot ]; then export KBENCH_HOT=1; fi
  rocprofv3 --kernel-trace --output-format csv -d $OUT/kbv_$mode -- python3 tools/kbench.py $CASE 12 > $OUT/kbv_$mode.log 2>&1
  echo "== $CASE $mode"; python3 profiles/analyze_trace.py $(ls $OUT/kbv_$mode/*/*kernel_trace.csv | head -1) 12 | grep -i "gemv"
  rm -rf $OUT/kbv_$mode
done
echo "logs: $OUT/kbv_cold.log $OUT/kbv_hot.log"
