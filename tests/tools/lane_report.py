"""Scalar-spill lane operations of a kernel by source line, from the compiler's own output (not a pytest; needs hipcc only, no GPU): the sibling of
tests/tools/spill_report.py, which counts v_readlane / v_writelane per kernel and lists `scratch_` instructions by line.  One kernel file is compiled to gfx950
assembly with the product's flags plus line tables, and for every kernel whose demangled name starts with the given fragment each v_readlane / v_writelane is
listed under the innermost source line it was generated for and the chain of calls that line was inlined through.  What a v_readlane restores is a
wave-uniform value that did not fit the scalar registers at that line: the table says which values to stop holding (profiles/r14_whole_uniforms_ab.md).
    python tests/tools/lane_report.py ['k_whole<false, false, true>'] [--file kernels_whole.hip] [--md profiles/NAME.md | --append profiles/NAME.md] [-DVPT_X=0 ...]
    (-D definitions are passed to the compiler: the A/B switches of tests/tools/build_variant.py)"""
import collections, importlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
B = importlib.import_module("vulkan-path-tracer_amd._build")
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")


def short_loc(x):
    """file:line of a line-table entry: the column goes, and so does where the compiler's own headers are installed"""
    return re.sub(r"^.*/include/hip/", "hip/", re.sub(r":\d+$", "", x.strip().replace("vulkan-path-tracer_amd/csrc/", "")))


def lane_ops(src, defs=()):
    """{demangled kernel name: Counter of 'read  <chain>' / 'write <chain>'}, chain = innermost line < the calls it was inlined through"""
    flags = [f for f in B.FLAGS if f != "-fPIC"] + ["-DVPT_LAB=0"] + list(defs) + B.EXTRA_FLAGS.get(src, []) + ["-gline-tables-only"]
    out = tempfile.mktemp(suffix=".s")
    subprocess.run([B.hipcc(), "-S", "--cuda-device-only", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(CSRC, src)] + flags,
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n"); os.unlink(out)
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:\s+; @", l)]
    demangled = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for k, ((i, _), (j, _)) in enumerate(zip(starts, starts[1:] + [(len(lines), "")])):
        chain, lanes = "", collections.Counter()
        for x in lines[i:j]:
            if ".loc" in x and ";" in x:
                chain = " < ".join(short_loc(q.strip(" ]")) for q in x.split(";")[-1].strip().split(" @["))
            if "v_readlane" in x or "v_writelane" in x:
                lanes[("write " if "v_writelane" in x else "read  ") + chain] += 1
        res[re.sub(r"\(.*", "", demangled[k].replace("(anonymous namespace)::", "")).replace("void ", "").replace("vpt::", "")] = lanes
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    defs = [a for a in args if a.startswith("-D")]
    src = opt("--file", "kernels_whole.hip")
    taken = {opt("--file", None), opt("--md", None), opt("--append", None)}
    frags = [a for a in args if not a.startswith("-") and a not in taken] or ["k_whole<false, false, true>"]
    out = []
    for name, lanes in lane_ops(src, defs).items():
        if any(name.startswith(f) for f in frags):
            out += ["Scalar-spill lane operations of `%s` (%s, source id %s%s) by source line — innermost line < the calls it was inlined through; %d reads, %d writes:"
                    % (name, src, B.source_id(), ", built with " + " ".join(defs) if defs else "", sum(c for w, c in lanes.items() if w.startswith("read")),
                       sum(c for w, c in lanes.items() if w.startswith("write"))), "", "| count | op | where |", "|---|---|---|"]
            out += ["| %d | %s | %s |" % (c, w[:5].strip(), w[6:]) for w, c in sorted(lanes.items(), key=lambda kv: (-kv[1], kv[0]))] + [""]
    text = "\n".join(out)
    if "--md" in args:
        open(os.path.join(ROOT, opt("--md", None)), "w").write(text)
    if "--append" in args:
        open(os.path.join(ROOT, opt("--append", None)), "a").write("\n" + text)
    print(text)
