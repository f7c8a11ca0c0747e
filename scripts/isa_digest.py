"""Did a source edit move a kernel?  Compares two device listings kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S vima_amd/csrc/gemm.hip -o new.s    (and the base tree's -> old.s)
    python scripts/isa_digest.py old.s new.s [--rename REGEX REPL]... [--remarks OLD NEW] [--table FILE]

Per kernel symbol: sha1 of its instruction stream with comments, directives and the function index inside .LBBn_m labels
removed (register numbers, immediates, label order all count). --rename rewrites the NEW listing's symbol names before the
comparison, for edits that change mangled names on purpose; e.g. after gemm_kernel gained the trailing template flag X3 and
gemm_x3_kernel became gemm_kernel<float, ..., X3>:

    --rename '11gemm_kernelIf(\\S*)ELb0ELb1(EEEvNS0_7GemmDevE)$' '14gemm_x3_kernelI\\1\\2' --rename '(11gemm_kernelI\\S*)ELb0(EEEvNS0_7GemmDevE)$' '\\1\\2'

and after attn_x3_kernel<D, MODE> became attn_mfma_kernel<D, MODE, X3 = true>:

    --rename '16attn_mfma_kernelI(\\S*)ELb1E(EEvNS0_7AttnDevE)$' '14attn_x3_kernelI\\1E\\2' --rename '(16attn_mfma_kernelI\\S*)ELb0E(EEvNS0_7AttnDevE)$' '\\1E\\2'

The digest ignores directives, so an edit that only changes a kernel's static LDS passes it: --remarks takes the two compiles'
-Rpass-analysis=kernel-resource-usage output (their stderr) and compares each kernel's table (registers, scratch, occupancy, LDS)
under the same renames.

Exit status 1 when a kernel present in both listings differs (digest or resources) or a kernel exists in one of them only. It is a
script and not a test because it needs the base tree's listing."""
import argparse
import hashlib
import re
import sys


def digests(path):
    src = open(path).read()
    out = {}
    c_kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", src, flags=re.M))   # extern "C" kernels have no _Z name (widen_kernel of vima_api.hip)
    for m in re.finditer(r"^([A-Za-z_]\S*):\s*;? ?@?.*$", src, flags=re.M):
        end = src.find(".Lfunc_end", m.end())
        if end < 0 or not (m.group(1).startswith("_Z") or m.group(1) in c_kernels):
            continue
        body = []
        for ln in src[m.end():end].split("\n"):
            t = "" if ln.strip().startswith(";;#ASM") else ln.split(";")[0].strip()
            if t and (not t.startswith(".") or re.match(r"\.LBB\d+_\d+:", t)):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        out[m.group(1)] = (hashlib.sha1("\n".join(body).encode()).hexdigest()[:12], len(body))
    return out


def resources(path):
    """{kernel: {field: value}} of a -Rpass-analysis=kernel-resource-usage log"""
    out, cur = {}, None
    for m in re.finditer(r"remark:\s+([^:\n]+): (\S+) \[-Rpass-analysis", open(path).read()):
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def renamed(table, rules):
    new = {}
    for name, d in table.items():
        for rx, repl in rules:
            name, n = re.subn(rx, repl, name)
            if n:
                break
        assert name not in new, f"--rename maps two kernels to {name}"
        new[name] = d
    return new


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--remarks", nargs=2, metavar=("OLD", "NEW"), help="the two compiles' kernel-resource-usage remarks: compare them too")
    ap.add_argument("--table", help="write 'symbol old-digest old-lines new-digest new-lines' per kernel to this file")
    args = ap.parse_args()
    old, new = digests(args.old), renamed(digests(args.new), args.rename)
    both = sorted(set(old) & set(new))
    diff = [k for k in both if old[k] != new[k]]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"{len(old)} kernels in {args.old}, {len(new)} in {args.new}: {len(both) - len(diff)} identical, {len(diff)} different, "
          f"{len(only_old)} only in the first, {len(only_new)} only in the second")
    for k in diff:
        print("  differs:", k, old[k], new[k])
    for k in only_old:
        print("  only in the first:", k)
    for k in only_new:
        print("  only in the second:", k)
    rdiff, rnote = [], ""
    if args.remarks:
        ro, rn = resources(args.remarks[0]), renamed(resources(args.remarks[1]), args.rename)
        rdiff = sorted(k for k in set(ro) | set(rn) if ro.get(k) != rn.get(k))
        rnote = f"resource tables: {len(ro)} kernels in {args.remarks[0]}, {len(rn)} in {args.remarks[1]}, {len(rdiff)} different"
        print(rnote)
        for k in rdiff:
            print("  resources differ:", k, ro.get(k), rn.get(k))
    if args.table:
        with open(args.table, "a") as f:
            f.write(f"# {args.old} -> {args.new}: symbol, old digest, old instruction lines, new digest, new instruction lines\n")
            for k in sorted(set(old) | set(new)):
                o, n = old.get(k, ("-", 0)), new.get(k, ("-", 0))
                f.write(f"{k} {o[0]} {o[1]} {n[0]} {n[1]}{'' if o == n else '   <-- DIFFERENT'}\n")
            f.write(f"# {rnote}{''.join(' ' + k for k in rdiff)}\n" if rnote else "")
    return 1 if diff or only_old or only_new or rdiff else 0


if __name__ == "__main__":
    sys.exit(main())
