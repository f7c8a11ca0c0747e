"""The rows that hold launch_gemm's kernel selection (vima_amd/csrc/gemm_route.h) to what it was recorded to be.

A row is data: the integers of a VimaGemmDesc (include/vima_hip.h), for each pointer `null` or its byte offset from a 256-byte
boundary, the handle's precision and its GEMM options. rows() lists

  * every (Case, options) of tests/gemm_forms_reference.py: gpu_cases(), and sweep_cases() under every knob setting of SWEEP;
  * both sides of every threshold the route has (threshold_rows: the smallest shape that sits on each);
  * one refusal per refusing condition that a VimaGemmDesc can reach (refusal_rows).

tests/golden/gemm_routes.json holds, per row, what vima_op_gemm returned for it on an MI355X BEFORE gemm_route.h existed (the
return class and GemmArgs::kernel_id), and the table of the seven gemm_*_ok predicates over predicate_grid(). Run as a program
(`python -m tests.gemm_route_cases record OUT.json`) this module is the recorder: it launches every row on buffers it allocates
itself, sized by buffer_bytes(); contents do not matter to routing (only grp_col is read by a kernel to find its columns and is filled).

fp8 operands (GemmArgs::a8 / w8) cannot be reached through vima_op_gemm and have no rows here: they are held by the gemm_a8_ok /
gemm_headmajor_ok(a8 = 1) columns of the predicate table, by tests/test_fp8_gpu.py and by whole-model launch logs."""
import hashlib
import json
import os
import sys

from tests import gemm_forms_reference as R

PTRS = ("A", "W", "A2", "W2", "mul", "resT", "outT", "outT_lo", "bias", "res", "rs_ssq", "rs_sum", "rs_c", "out32", "ssq_out", "sum_out", "grp_col")
T_PTRS = ("A", "W", "A2", "W2", "mul", "resT", "outT", "outT_lo")   # buffers in the handle's operand type; the rest are 4-byte elements
I64 = ("bsA", "bsW", "bsBias", "bsMul", "bsRes", "bs32", "bsT")
I32 = ("M", "N", "K", "lda", "ldw", "lda2", "ldw2", "ldmul", "ldres", "ldresT", "ld32", "ldT", "ldT_lo", "batch", "act",
       "hm_D", "hm_L", "pair32", "rb", "s_hi", "s_lo", "ro", "split_n", "rs_parts", "x3")
# Tuning fields in the order the CPU driver (tests/gemm_route_driver.cpp) reads them; -1 = process default
KNOBS = ("gemm_variant", "gemm_tile", "gemm_raster", "gemm_epi", "gemm_persist", "gemm_small", "gemm_wide", "gemm_pp", "gemm_q4", "gemm_splitk",
         "gemm_resident", "gemm_res_maxwg", "gemm_skinny", "gemm_flat", "gemm_res_nch")
SLACK = 4096   # elements behind every buffer's computed extent
# kernel families (kernel_id / 1000) the non-lab launcher can emit through vima_op_gemm
FAMILIES = (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 15, 16, 17, 18, 19, 20, 21, 23)


def row(name, M, N, K, prec="bf16", opts=None, ptrs=None, grp=None, **ints):
    """A dense bf16 problem with a bf16 output at ld = its width unless said otherwise. ptrs: {name: byte offset} ADDED to A, W (and
    outT unless another output is named or outT is given as None)."""
    d = dict.fromkeys(I64 + I32, 0)
    d.update(M=M, N=N, K=K, lda=K, ldw=K, batch=1)
    d.update(ints)
    p = {"A": 0, "W": 0}
    p.update(ptrs or {})
    if not any(k in p for k in ("outT", "out32")):
        p["outT"] = 0
    p = {k: v for k, v in p.items() if v is not None}
    width = N // 2 if d["pair32"] else N
    for ptr, ld in (("outT", "ldT"), ("out32", "ld32"), ("mul", "ldmul"), ("res", "ldres"), ("resT", "ldresT")):
        if ptr in p and not d[ld]:
            d[ld] = width - d["split_n"] if ptr == "outT" else (N if ptr in ("mul", "res", "resT") else width)
    if "outT_lo" in p and not d["ldT_lo"]:
        d["ldT_lo"] = d["split_n"]
    r = {"name": name, "prec": prec, "opts": dict(opts or {}), "d": d, "p": p}
    if grp:
        r["grp"] = list(grp)
    return r


def from_case(c, opts, name=None):
    """The row of a gemm_forms_reference.Case: field for field what tests/test_gemm_forms_gpu.py passes for it."""
    batched = c.batch > 1 and c.grp is None
    wrows = c.grp[-1] if c.grp is not None else c.N
    rows_out = max(c.orow(r) for r in range(c.M)) + 1 + c.gap
    ints = dict(lda=c.lda, ldw=c.ldw, batch=c.batch, act=c.act,
                bsA=(c.M + c.gap) * c.lda if c.batch > 1 else 0, bsW=(wrows + c.gap) * c.ldw if batched else 0,
                bsBias=wrows + 4 * (c.gap > 0) if (c.bias and batched) else 0,
                bsMul=(c.M + c.gap) * c.ldmul if (c.mul and c.batch > 1) else 0, bsRes=(c.M + c.gap) * c.ldres if (c.res and c.batch > 1) else 0,
                bs32=rows_out * c.ld32 if (batched and c.out32) else 0, bsT=rows_out * c.ldT if (batched and c.outT) else 0,
                pair32=int(c.pair32), split_n=c.split_n, x3=int(c.prec == "bf16x3"))
    p = {"outT": 0 if c.outT else None}
    if c.dual:
        p["W2"], p["A2"] = 0, 0
        ints.update(ldw2=c.ldw2, lda2=c.lda2 if c.dual == "sep" else c.lda)
    for flag, ptr, ld in ((c.bias, "bias", None), (c.mul, "mul", "ldmul"), (c.res, "res", "ldres"), (c.resT, "resT", "ldresT"),
                          (c.out32, "out32", "ld32"), (c.outT, "outT", "ldT"), (c.split_n, "outT_lo", "ldT_lo"), (c.ssq, "ssq_out", None),
                          (c.sumo, "sum_out", None), (c.rs, "rs_ssq", None), (c.rs == "ln", "rs_sum", None), (c.rs == "ln", "rs_c", None),
                          (c.grp is not None, "grp_col", None)):
        if flag:
            p[ptr] = 0
            if ld:
                ints[ld] = getattr(c, ld)
    if c.hm:
        ints["hm_D"], ints["hm_L"] = c.hm
    if c.remap:
        ints["rb"], ints["s_hi"], ints["s_lo"], ints["ro"] = c.remap
    if c.rs:
        ints["rs_parts"] = c.rs_parts
    return row(name or c.name, c.M, c.N, c.K, prec=c.prec, opts=opts, ptrs=p, grp=c.grp, **ints)


def form_rows():
    out = [from_case(c, opts) for _, c, opts, _ in R.gpu_cases()]
    for form, c, base in R.sweep_cases():
        for knobs in R.SWEEP:
            opts = dict(base)
            opts.update(knobs)
            name = f"sweep {form} {sorted(opts.items())}"
            if name not in [r["name"] for r in out]:   # (a form whose base options already hold the swept knob)
                out.append(from_case(c, opts, name=name))
    return out


def threshold_rows():
    out = []

    def add(name, *a, **kw):
        out.append(row("edge " + name, *a, **kw))

    # the `large` rule: 150 / 160 tiles of 256x256, and a ragged M either side of waste 1.15 (5 x 32 tiles: 1280 / M < 1.15 from M = 1114 on)
    add("150 tiles", 2560, 3840, 128)
    add("160 tiles", 2560, 4096, 128)
    add("waste 1.15004", 1113, 8192, 128)
    add("waste 1.14901", 1114, 8192, 128)
    # underfilled 128x128 grids: 120 / 128 tiles
    add("t128 120", 1024, 1920, 128)
    add("t128 128", 1024, 2048, 128)
    for M in (32, 33):
        add(f"M {M}", M, 768, 768)
        add(f"M {M} skinny off", M, 768, 768, opts={"gemm_skinny": 0})
    # launch_resident: the three grid steps 32x32 -> 64x32 -> 64x64 -> declined, at gemm_res_maxwg 256 (default) and 8
    for maxwg, shapes in ((256, [(64, 4096), (64, 4128), (64, 8192), (64, 8224), (128, 8192), (128, 8256)]),
                          (8, [(64, 128), (64, 160), (64, 256), (64, 288), (128, 256), (128, 320)])):
        for M, N in shapes:
            add(f"resident maxwg {maxwg} {M}x{N}", M, N, 128, opts={"gemm_res_maxwg": maxwg})
    for N in (1024, 1056):   # at most 32 rows without the skinny kernel: n32 * batch <= 4 * maxwg
        add(f"resident 32 rows maxwg 8 N {N}", 32, N, 128, opts={"gemm_res_maxwg": 8, "gemm_skinny": 0})
    for K in (64, 128, 192, 256):   # full tiles: one K-slice (one-tile kernel), even / odd slice counts (ping-pong / round-2 loop)
        add(f"K {K}", 2560, 4096, K)
    for opts in ({"gemm_q4": 1}, {"gemm_q4": 2}, {"gemm_q4": 3}, {"gemm_wide": 1}):
        for M, N in ((3328, 3840), (3328, 4096), (16384, 768), (16384, 1024)):
            add(f"N % 384 {M}x{N} {opts}", M, N, 128, opts=opts)
    for M in (32512, 32768):
        add(f"q4 6 M {M}", M, 768, 128, opts={"gemm_q4": 6})
        add(f"q4 default M {M}", M, 768, 128)
    # GEGLU pair either side of gemm_pair_large (>= 160 full tiles of the interleaved problem, an even number of K-slices)
    for M, N, K in ((2560, 4096, 128), (2560, 3840, 128), (2560, 4096, 192)):
        add(f"pair32 {M}x{N}x{K}", M, N, K, pair32=1, act=R.ACT_GELU, ptrs={"bias": 0})
    for q4 in (1, 2):
        for L in (256, 128):
            add(f"head-major L {L} q4 {q4}", 3328, 3840, 128, opts={"gemm_q4": q4}, hm_D=64, hm_L=L)
    add("head-major L 256 default knobs", 3328, 3840, 128, hm_D=64, hm_L=256)
    add("outT 4 bytes off (scalar epilogue)", 70, 136, 320, ptrs={"outT": 4}, ldT=136)
    add("outT 4 bytes off, large", 2560, 4096, 128, ptrs={"outT": 4})
    add("ldT % 8 != 0 (no 8-column epilogue)", 2560, 4096, 128, ldT=4100)
    add("ldT % 8 != 0, small", 70, 136, 320, ldT=140)
    add("bf16 stream, large", 2560, 4096, 128, ptrs={"resT": 0})
    add("fp32 stream, large", 2560, 4096, 128, ptrs={"res": 0, "out32": 0, "outT": 0})
    add("gate, large", 2560, 4096, 128, act=R.ACT_GELU, ptrs={"mul": 0})
    add("gate with relu, large (no specialised epilogue)", 2560, 4096, 128, act=R.ACT_RELU, ptrs={"mul": 0})
    add("batched, large", 256, 256, 128, batch=160, bsA=256 * 128, bsW=256 * 128, bsT=256 * 256)
    add("nothing to do", 0, 128, 64)
    for t in (13, 14):   # the two lab tiles report no kernel_id
        add(f"gemm_tile {t}", 70, 136, 320, opts={"gemm_tile": t})
    add("fp32 large", 512, 512, 128, prec="fp32", ptrs={"out32": 0})
    return out


def refusal_rows():
    out = []

    def add(name, *a, **kw):
        out.append(row("refuse " + name, *a, **kw))

    big = {"gemm_tile": 2}
    add("K not a multiple of the slice", 70, 136, 96)
    add("K zero", 70, 136, 0)
    add("x3 on a bf16 handle", 70, 136, 320, x3=1)
    add("A misaligned", 70, 136, 320, ptrs={"A": 8})
    add("lda not 16 bytes", 70, 136, 320, lda=324)
    add("grouped with an activation", 5, 100, 64, batch=4, grp=[0, 100, 150, 157, 158], ld32=160, ptrs={"out32": 0, "grp_col": 0}, act=R.ACT_RELU)
    add("grouped at gemm_tile 1", 5, 100, 64, batch=4, grp=[0, 100, 150, 157, 158], ld32=160, ptrs={"out32": 0, "grp_col": 0}, opts={"gemm_tile": 1})
    add("dual without A2", 21, 100, 64, act=R.ACT_GELU, ldw2=64, ldT=104, ptrs={"W2": 0})
    add("dual too large for one grid", 2560, 4096, 128, act=R.ACT_GELU, ldw2=128, lda2=128, ptrs={"W2": 0, "A2": 0})
    add("dual with relu", 70, 100, 64, act=R.ACT_RELU, ldw2=64, lda2=64, ldT=104, ptrs={"W2": 0, "A2": 0})
    add("dual, output 4 bytes off", 70, 100, 64, act=R.ACT_GELU, ldw2=64, lda2=64, ldT=104, ptrs={"W2": 0, "A2": 0, "outT": 4})
    add("both residuals", 70, 136, 320, ptrs={"res": 0, "resT": 0})
    add("bf16 residual with an activation", 70, 136, 320, act=R.ACT_RELU, ptrs={"resT": 0})
    add("head-major on a small problem", 1024, 256, 128, hm_D=64, hm_L=256)
    add("head-major, head not a power of two", 1024, 256, 128, opts=big, hm_D=48, hm_L=256)
    add("head-major with an activation", 1024, 256, 128, opts=big, hm_D=64, hm_L=256, act=R.ACT_RELU)
    add("head-major, ldT % 8 != 0", 1024, 256, 128, opts=big, hm_D=64, hm_L=256, ldT=260)
    add("head-major with fp32 output", 1024, 256, 128, opts=big, hm_D=64, hm_L=256, ptrs={"out32": 0, "outT": 0})
    add("head-major on the one-tile kernel", 1024, 256, 128, opts={"gemm_tile": 2, "gemm_persist": 0}, hm_D=64, hm_L=256)
    add("sum_out without ssq_out", 70, 96, 320, ptrs={"out32": 0, "sum_out": 0})
    add("sum_out on a large problem", 2560, 4096, 128, ptrs={"out32": 0, "ssq_out": 0, "sum_out": 0})
    add("rs_sum without rs_c", 70, 384, 64, pair32=1, act=R.ACT_GELU, rs_parts=2, ptrs={"rs_ssq": 0, "rs_sum": 0}, opts={"gemm_small": 0})
    add("rs_sum on a plain GEMM", 70, 136, 320, rs_parts=2, ptrs={"rs_ssq": 0, "rs_sum": 0, "rs_c": 0})
    add("ssq_out with N % 32 != 0", 70, 136, 320, ptrs={"out32": 0, "ssq_out": 0})
    add("ssq_out without an output", 70, 96, 320, ptrs={"outT": None, "ssq_out": 0, "out32": None})
    add("ssq_out of bf16 values without the 8-column epilogue", 70, 96, 320, ldT=100, ptrs={"ssq_out": 0})
    add("rs_ssq with no partials", 70, 136, 320, ptrs={"rs_ssq": 0})
    add("split_n not a multiple of 128", 70, 264, 320, split_n=64, ptrs={"outT_lo": 0})
    add("split_n with fp32 output", 70, 264, 320, split_n=128, ptrs={"outT_lo": 0, "out32": 0, "outT": 0})
    add("split_n under split-K", 70, 264, 320, split_n=128, ptrs={"outT_lo": 0}, opts={"gemm_splitk": 1})
    add("pair32 with relu", 70, 384, 64, pair32=1, act=R.ACT_RELU, opts={"gemm_small": 0})
    add("pair32 where the dual form is the one to use", 70, 384, 64, pair32=1, act=R.ACT_GELU)
    add("pair32 on an fp32 handle", 70, 384, 64, prec="fp32", pair32=1, act=R.ACT_GELU, opts={"gemm_small": 0})
    add("pair32 with N % 128 != 0", 70, 320, 64, pair32=1, act=R.ACT_GELU, opts={"gemm_small": 0})
    return out


def rows():
    out = form_rows() + threshold_rows() + refusal_rows()
    names = [r["name"] for r in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


def elem_size(r, ptr):
    return (2 if r["prec"] == "bf16" else 4) if ptr in T_PTRS else 4


def buffer_bytes(r):
    """{pointer: bytes to allocate behind it}: the extent the launch can touch, plus SLACK elements."""
    d = r["d"]
    M, N, nb = d["M"], d["N"], max(d["batch"], 1)
    grp = r.get("grp")
    wrows = grp[-1] if grp else N
    width = N // 2 if d["pair32"] else N
    orow = (lambda i: (i // d["rb"]) * d["s_hi"] + (i % d["rb"]) * d["s_lo"] + d["ro"]) if d["rb"] else (lambda i: i)
    rows_out = max([orow(i) for i in range(M)] or [0]) + 1
    ext = {"A": (nb - 1) * d["bsA"] + M * d["lda"], "W": (nb - 1) * d["bsW"] + wrows * d["ldw"], "A2": M * d["lda2"], "W2": N * d["ldw2"],
           "mul": (nb - 1) * d["bsMul"] + M * d["ldmul"], "res": (nb - 1) * d["bsRes"] + M * d["ldres"], "resT": M * d["ldresT"],
           "bias": (nb - 1) * d["bsBias"] + wrows, "rs_ssq": M * max(d["rs_parts"], 1), "rs_sum": M * max(d["rs_parts"], 1), "rs_c": N,
           "out32": (nb - 1) * d["bs32"] + rows_out * max(d["ld32"], width), "ssq_out": M * (N // 32 + 1), "sum_out": M * (N // 32 + 1),
           "outT": max((nb - 1) * d["bsT"] + rows_out * max(d["ldT"], width - d["split_n"]), M * N if d["hm_D"] else 0),
           "outT_lo": M * max(d["ldT_lo"], d["split_n"]), "grp_col": nb + 1}
    return {k: (max(ext[k], 0) + SLACK) * elem_size(r, k) for k in r["p"]}


# ------------------------------------------------------------------------------------------------ the predicate table
GRID_M = (1, 32, 33, 255, 256, 2304, 2560, 16384, 32768, 131072)
GRID_N = (64, 96, 768, 1536, 2304, 3072, 4096)
GRID_K = (64, 128, 192, 256, 768, 3072)
GRID_PAD = (0, 8)   # leading dimensions K and K + 8
HM = ((64, 256), (64, 512), (64, 128), (48, 256))   # (hm_D, hm_L) of the gemm_headmajor_ok columns, each at a8 = 0 and 1
PREDICATES = (["pair_large", "pair_ok", "lnfold_producer_ok", "dual_ok", "a8_ok", "grouped_ok"] +
              [f"headmajor_ok {D} {L} {a8}" for D, L in HM for a8 in (0, 1)])


def predicate_knobs():
    """Default knobs, then each routing knob moved alone to every value gemm_forms_reference.SWEEP uses (and gemm_res_maxwg 8, gemm_q4 3)."""
    out = [{}]
    for s in R.SWEEP:
        if len(s) == 1 and s not in out and s != {"gemm_tile": 0}:
            out.append(dict(s))
    return out + [{"gemm_tile": 0}, {"gemm_res_maxwg": 8}, {"gemm_q4": 3}]


def predicate_grid():
    return [(M, N, K, K + pad) for M in GRID_M for N in GRID_N for K in GRID_K for pad in GRID_PAD]


def knob_vector(opts):
    return [int(opts.get(k, -1)) for k in KNOBS]


def driver_lines(route_rows, ncu):
    """stdin of tests/gemm_route_driver.cpp for the launch rows, one line each."""
    out = []
    for r in route_rows:
        d = r["d"]
        f = ["R", ncu, int(r["prec"] == "bf16")] + knob_vector(r["opts"]) + [d[k] for k in I64 + I32] + [r["p"].get(k, -1) for k in PTRS]
        out.append(" ".join(str(x) for x in f))
    return out


def predicate_lines():
    """... and for the predicate table: one line per (knobs, grid point); the driver answers with one character per entry of PREDICATES."""
    out = []
    for opts in predicate_knobs():
        kv = " ".join(str(x) for x in knob_vector(opts))
        for M, N, K, ld in predicate_grid():
            out.append(f"P {kv} {M} {N} {K} {ld} {ld} " + " ".join(f"{D} {L}" for D, L in HM))
    return out


# ------------------------------------------------------------------------------------------------ the recorder (GPU)
def err_class(rc):
    return 0 if rc == 0 else ("invalid" if rc == 1 else "other")   # 1 = hipErrorInvalidValue


def launch_rows(route_rows):
    """Every row through vima_op_gemm on buffers allocated here; -> [(return class, kernel_id)]."""
    import ctypes
    import torch
    from vima_amd import _lib
    from tests.gpu_common import bare_policy
    out = []
    for r in route_rows:
        pol = bare_policy(r["prec"])
        keep, d = [], _lib.VimaGemmDesc()
        for k, nbytes in buffer_bytes(r).items():
            off = r["p"][k]
            buf = torch.zeros(nbytes + 512 + off, dtype=torch.uint8, device="cuda:0")
            base = (buf.data_ptr() + 255) // 256 * 256
            assert base + off + nbytes <= buf.data_ptr() + buf.numel()
            if k == "grp_col" and r.get("grp"):
                col = torch.tensor(r["grp"], dtype=torch.int32, device="cuda:0").view(torch.uint8)
                buf[base - buf.data_ptr() + off:][:col.numel()] = col
            keep.append(buf)
            setattr(d, k, base + off)
        for k, v in r["d"].items():
            setattr(d, k, v)
        d.rs_invk, d.rs_eps = 1.0 / max(r["d"]["K"], 1), 1e-5
        for k, v in r["opts"].items():
            pol.set_option(k, v)
        try:
            kid = ctypes.c_int(0)
            rc = pol._lib.vima_op_gemm(pol._handle, ctypes.byref(d), ctypes.byref(kid), pol._stream())
            torch.cuda.synchronize()
        finally:
            for k in r["opts"]:
                pol.set_option(k, -1)
        out.append((err_class(rc), kid.value))
        del keep
    return out


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.json")


def rows_sha1(rs):
    return hashlib.sha1(json.dumps(rs, sort_keys=True).encode()).hexdigest()


def golden(path=GOLDEN):
    """The table as the tests use it: {"num_cu", "rows_sha1", "routes": [(return class, kernel_id)] in the order of rows(), "predicates": [{predicate:
    one 0/1 character per point of predicate_grid()}] in the order of predicate_knobs()}. In the file a route is its kernel_id, or "class:kernel_id" for a
    refusal; a predicate column is an index into "predicate_columns" (hex of its bits, first grid point = highest bit): there are only 16 different ones."""
    with open(path) as f:
        g = json.load(f)
    n = len(predicate_grid())
    cols = [format(int(h, 16), "0%db" % n) for h in g["predicate_columns"]]
    g["routes"] = [(0, x) if isinstance(x, int) else (x.split(":")[0], int(x.split(":")[1])) for x in g["routes"]]
    g["predicates"] = [dict(zip(PREDICATES, (cols[i] for i in line))) for line in g["predicates"]]
    return g


def record(path):
    """Launches rows() and writes their results; the predicate sections of an existing file are kept (they were tabulated on the CPU from the
    predicates' bodies of the recorded commit)."""
    rs = rows()
    res = [kid if rc == 0 else f"{rc}:{kid}" for rc, kid in launch_rows(rs)]
    old = {}
    try:
        with open(path) as f:
            old = json.load(f)
    except (OSError, ValueError):
        pass
    with open(path, "w") as f:
        f.write('{\n"num_cu": %d,\n"rows_sha1": "%s",\n"routes": [\n' % (num_cu(), rows_sha1(rs)))
        f.write(",\n".join(json.dumps(res[i:i + 24])[1:-1] for i in range(0, len(res), 24)))
        f.write('\n],\n"predicate_columns": [\n' + ",\n".join(json.dumps(c) for c in old.get("predicate_columns", [])))
        f.write('\n],\n"predicates": [\n' + ",\n".join(json.dumps(t) for t in old.get("predicates", [])) + "\n]\n}\n")
    print(f"recorded {len(rs)} rows on {num_cu()} CUs -> {path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    else:
        sys.exit("usage: python -m tests.gemm_route_cases record OUT.json")
