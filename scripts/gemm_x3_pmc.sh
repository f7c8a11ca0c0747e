#!/bin/bash
# What bounds gemm_kernel<float, ..., X3> (precision "bf16x3"): matrix-pipe and vector-issue counters of ONE split-bf16 GEMM launched through
# vima_op_linear on a bf16x3 handle (default shape: the T5 qkv GEMM of VIMA-200M at batch 32, M = 16384, N = 2304, K = 768).
# Separate small --pmc passes, each under its own time limit, kernel trace only. Usage: bash scripts/gemm_x3_pmc.sh OUTDIR [M N K]
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:?output directory}; shift
SHAPE=${*:-16384 2304 768}
mkdir -p "$OUT"
DRIVER="import sys, torch; sys.path.insert(0, '$R')
from vima_amd import _lib; from tests.gpu_common import bare_policy, ptr
M, N, K = map(int, sys.argv[1:4]); pol = bare_policy('bf16x3'); g = torch.Generator().manual_seed(0)
A = torch.randn(M, K, generator=g).cuda(); W = (torch.randn(N, K, generator=g) * K ** -0.5).cuda(); out = torch.empty(M, N, device='cuda')
for _ in range(2): _lib.check(pol._lib.vima_op_linear(pol._handle, ptr(A), ptr(W), None, None, None, M, N, K, 0, ptr(out), pol._stream()))
torch.cuda.synchronize()"
pass() {  # pass <name> <counters...>
  local name=$1; shift
  rm -rf "$OUT/$name"
  timeout -k 10 120 rocprofv3 --kernel-trace --pmc "$@" -d "$OUT/$name" -o p --output-format csv -- python -c "$DRIVER" $SHAPE > "$OUT/$name.log" 2>&1
  local rc=$?
  case $rc in 124|134|137|139) echo "pass $name: rc $rc, stopping"; exit $rc;; esac
}
pass a GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES
pass b SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVES
pass c SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_WAIT_ANY
python3 - "$OUT" $SHAPE <<'PY'
import csv, glob, re, sys, collections
out, M, N, K = sys.argv[1], *map(int, sys.argv[2:5])
acc = collections.defaultdict(list)
for f in glob.glob(f"{out}/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if re.search(r"gemm_kernel<float,.*, false, true>", r["Kernel_Name"]):   # W8 = false, X3 = true
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
c = {k: sum(v) / len(v) for k, v in acc.items()}
print(f"gemm_kernel<float, ..., X3>, M = {M}, N = {N}, K = {K}; per-dispatch means of the chip-summed counters:")
for k in sorted(c):
    print(f"  {k} {c[k]:.6g}")
need = ("GRBM_GUI_ACTIVE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_INSTS_VALU", "SQ_WAVES")
if all(k in c for k in need):
    simds = 256 * 4
    mfma = c["SQ_VALU_MFMA_BUSY_CYCLES"] / 32               # 32 cycles per v_mfma_f32_32x32x16_bf16
    tiles = ((M + 127) // 128) * ((N + 127) // 128); slices = K // 32
    elapsed = c["GRBM_GUI_ACTIVE"] / 8                         # GRBM_GUI_ACTIVE is summed over the 8 XCDs
    print(f"  MFMA busy / (elapsed x SIMDs)                    {c['SQ_VALU_MFMA_BUSY_CYCLES'] / (elapsed * simds):.3f}")
    if "SQ_ACTIVE_INST_VALU" in c:                            # quad-cycles
        print(f"  VALU active / (elapsed x SIMDs)                  {4 * c['SQ_ACTIVE_INST_VALU'] / (elapsed * simds):.3f}")
    print(f"  MFMAs per wave and K-slice (expected 24)          {mfma / (tiles * 4 * slices):.2f}")
    print(f"  SQ_INSTS_VALU per wave and K-slice                {c['SQ_INSTS_VALU'] / (tiles * 4 * slices):.1f}")
    if "SQ_INSTS_LDS" in c:
        print(f"  SQ_INSTS_LDS per wave and K-slice                 {c['SQ_INSTS_LDS'] / (tiles * 4 * slices):.1f}")
PY
