"""What the compiler puts between the MFMAs of the exact-split K loops (csrc/split_core.h).  CPU only: compiles lstm.hip and gemm_ops.hip to
gfx950 assembly with the flags of csrc/Makefile, finds the main loop of every gemm_split_kernel<9, ...> and gemm_split_tn_kernel<...> (the
backward branch that encloses the most MFMAs) and prints, per loop: MFMA count, VALU count by mnemonic, LDS and VMEM counts.  Only mnemonics
that begin with v_, ds_, global_load and buffer_load are counted.  v_mov_b32 is broken down by its source (register / literal zero / other
constant) because the step kernels' full-step loop must hold neither of the first two.  With --resources the compiler's own report
(-Rpass-analysis=kernel-resource-usage) of the same kernels is printed too.

    python scripts/loop_isa.py [--resources] [--flags "-fno-slp-vectorize"] [--csrc DIR]      (profiles/split_loop_isa.txt)"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("lstm.hip", "gemm_ops.hip")
WANTED = ("gemm_split_kernel<9,", "gemm_split_tn_kernel<")


def makefile_flags(csrc):
    """HIPCC and CXXFLAGS of csrc/Makefile with $(ARCH) resolved."""
    var = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"(\w+)\s*\??=\s*(.*)", line)
        if m:
            var.setdefault(m.group(1), m.group(2).strip())
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def demangle(hipcc, names):
    filt = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def functions(asm):
    """name -> list of lines of every function of the assembly text"""
    fns, name, body = {}, None, []
    for line in asm.split("\n"):
        if name is None:
            m = re.match(r"(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            fns[name], name = body, None
        else:
            body.append(line)
    return fns


def main_loop(body):
    """the lines of the loop that holds the most MFMAs.  A loop is what ends in a backward branch to its header; the compiler's block
    comments (`Loop Header`, `in Loop: Header=BBn_m`) name the blocks between the two, which a rotated loop does not keep in one span."""
    loops, cur = collections.OrderedDict(), None
    for line in body:
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", line)
        if m:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", m.group(2))
            cur = m.group(1) if "Loop Header" in m.group(2) else h.group(1) if h else None
        if cur:
            loops.setdefault(cur, []).append(line)
    best = None
    for lines in loops.values():
        n = sum((l.split() or [""])[0].startswith("v_mfma") for l in lines)
        if n and (best is None or n > best[0]):
            best = (n, lines)
    return best[1] if best else None


def mov_kind(ops):
    src = ops.split(",")[-1].strip()
    if re.fullmatch(r"[vsa]\d+|[vsa]\[\d+:\d+\]|vcc_lo|vcc_hi|exec_lo|exec_hi|m0", src):
        return "register" if src[0] in "va" else "scalar register"
    return "zero" if src in ("0", "0x0") else "constant"


def count(lines):
    mf, valu, lds, vmem = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    for line in lines:
        for stmt in line.split(";")[0].split("\n"):
            tok = stmt.split(None, 1)
            if not tok or tok[0].endswith(":") or tok[0].startswith("."):
                continue
            mn, ops = re.sub(r"_e(32|64)$", "", tok[0]), tok[1] if len(tok) > 1 else ""
            if mn.startswith("v_mfma"):
                mf[mn] += 1
            elif mn.startswith("v_"):
                valu[mn + (" <- " + mov_kind(ops) if mn == "v_mov_b32" else "")] += 1
            elif mn.startswith("ds_"):
                lds[mn] += 1
            elif mn.startswith("global_load") or mn.startswith("buffer_load"):
                vmem[mn] += 1
    return mf, valu, lds, vmem


def resources(remarks, names):
    """mangled name -> {field: value} out of the compiler's kernel-resource-usage remarks"""
    res, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"remark:\s+(Function Name|[\w ]+?)(?: \[[\w/]+\])?: (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2) if m.group(2) in names else None
        elif cur:
            res.setdefault(cur, {})[m.group(1).strip()] = m.group(2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resources", action="store_true", help="also print the compiler's resource report of each kernel")
    ap.add_argument("--flags", default="", help="extra compiler flags (a build variant)")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "visdial_amd", "csrc"), help="source directory (another checkout's, to compare)")
    args = ap.parse_args()
    hipcc, flags = makefile_flags(args.csrc)
    flags += args.flags.split()
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for src in SOURCES:
            out = os.path.join(tmp, src.replace(".hip", ".s"))
            cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
            jobs.append((src, out, subprocess.Popen(cmd, cwd=args.csrc, stderr=subprocess.PIPE, text=True)))
        for src, out, proc in jobs:
            remarks = proc.communicate()[1]
            if proc.returncode:
                raise SystemExit("%s: the compiler failed\n%s" % (src, remarks[-2000:]))
            fns = functions(open(out).read())
            nice = demangle(hipcc, sorted(fns))
            names = [n for n in sorted(fns, key=lambda n: nice[n]) if any(w in nice[n] for w in WANTED)]
            res = resources(remarks, set(names)) if args.resources else {}
            for n in names:
                kernel = re.sub(r"^void |\(.*$", "", nice[n])
                loop = main_loop(fns[n])
                print("%s: %s" % (src, kernel))
                if loop is None:
                    print("  no loop with MFMAs")
                    continue
                mf, valu, lds, vmem = count(loop)
                nmf, nv = sum(mf.values()), sum(valu.values())
                print("  main loop: %d MFMA (%s), %d VALU (%.2f per MFMA), %d LDS, %d VMEM" % (
                    nmf, ", ".join("%d %s" % (c, k) for k, c in sorted(mf.items())), nv, nv / max(nmf, 1), sum(lds.values()), sum(vmem.values())))
                for title, cnt in (("VALU", valu), ("LDS", lds), ("VMEM", vmem)):
                    for k, c in sorted(cnt.items(), key=lambda kc: (-kc[1], kc[0])):
                        print("    %-5s %4d  %s" % (title, c, k))
                if n in res:
                    r = res[n]
                    print("  resources: %s VGPRs, %s AGPRs, scratch %s bytes/lane, occupancy %s waves/SIMD" % (
                        r.get("VGPRs"), r.get("AGPRs"), r.get("ScratchSize"), r.get("Occupancy")))


if __name__ == "__main__":
    main()
