"""tests/tools/asm_identity.py for a change that FOLDS one kernel file into another's translation unit (that tool compares file by file, so a kernel that
moved to another file reads as gone and new): kernels are matched by symbol across files, and a verdict is added for what a move alone changes.
Does the working tree compile to the same kernels as a git revision?  The check of a refactor (not a pytest; needs hipcc only, no GPU): every kernels_*.hip
of the revision (its csrc/ and include/ exported with git archive) and of the working tree is compiled to gfx950 assembly with the product's flags
(tests/tools/spill_report.py's compile line without line tables: source line numbers move in a refactor), and every kernel symbol is classified as
  identical  the same lines (lines that name the per-file __hip_cuid_ symbol are dropped);
  relabelled the same lines once the kernel's position in its file is taken out: local labels carry the function's number in its translation unit (.LBB13_2,
             .Lfunc_end13), and the directives that open the NEXT function trail a kernel's lines — both move when a file is folded into another;
  renamed    the same sequence of opcodes once every register operand is replaced by its class (v, s, a; vcc / exec as they are), and the same NumVgprs,
             TotalNumSgprs, ScratchSize, Occupancy and LDS size;
  differs    anything else, with the first differing line.
A kernels_*.hip that another one includes (a fold: one fat binary less, DESIGN.md "Library size") is no translation unit of its tree and is not compiled on
its own; a kernel is matched by its symbol, whichever file it was compiled in, and the table names both files where they differ.
Exit status 1 if any kernel differs.
    python tests/tools/asm_identity_folds.py <git-rev> [--lab] [--md profiles/NAME.md]"""
import concurrent.futures, importlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
B = importlib.import_module("vulkan-path-tracer_amd._build")
PKG = "vulkan-path-tracer_amd"
FIGURES = ("; NumVgprs:", "; TotalNumSgprs:", "; ScratchSize:", "; Occupancy:", "; LDSByteSize:")


def kernels(root, src, lab):
    """{kernel symbol: its lines} of one source file of the tree at root."""
    csrc = os.path.join(root, PKG, "csrc")
    flags = [f for f in B.FLAGS if f != "-fPIC"] + ["-DVPT_LAB=%d" % lab] + B.EXTRA_FLAGS.get(src, [])
    out = tempfile.mktemp(suffix=".s")
    subprocess.run([B.hipcc(), "-S", "--cuda-device-only", "-I" + csrc, "-I" + os.path.join(root, "include"), "-o", out, os.path.join(csrc, src)] + flags,
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    lines = [l for l in open(out).read().split("\n") if "__hip_cuid_" not in l]; os.unlink(out)
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:\s+; @", l)]
    end = next((i for i, l in enumerate(lines) if re.match(r"^\s+\.(set amdgpu\.|amdgpu_metadata|section\s+\.AMDGPU\.gpr_maximums)", l)), len(lines))   # what follows the file's last kernel
    return {n: lines[i:j] for (i, n), (j, _) in zip(starts, starts[1:] + [(end, "")])}


def shape(body):
    """A kernel's opcodes with every register operand reduced to its class, and its resource figures."""
    ops = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", l.split(";")[0]).split() for l in body if re.match(r"^\s+[a-z]\w*\s", l + " ")]
    return ops, [l.strip() for l in body if l.strip().startswith(FIGURES)]


def unplaced(body):
    """A kernel's lines without what depends on its position in the translation unit."""
    return [re.sub(r"\s+", " ", re.sub(r"(?:\.L|\b)(BB|func_end|func_begin)\d+", r"\1", l)) for l in body if not re.match(r"^\s+\.(text|section|protected|globl|weak|p2align|type|p2alignl|fill)\b", l)]   # (.p2alignl / .fill: the padding behind the file's last function)


def classify(old, new):
    if old is None or new is None:
        return "differs", "only in the %s" % ("working tree" if old is None else "revision")
    if old == new:
        return "identical", ""
    if unplaced(old) == unplaced(new):
        return "relabelled", ""
    first = next(("`%s` / `%s`" % (a.strip(), b.strip()) for a, b in zip(old, new) if a != b), "%d / %d lines" % (len(old), len(new)))
    return ("renamed" if shape(old) == shape(new) else "differs"), first


if __name__ == "__main__":
    rev, lab = sys.argv[1], int("--lab" in sys.argv)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, PKG + "/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        def kernel_files(root):
            csrc = os.path.join(root, PKG, "csrc")
            all_ = sorted(f for f in os.listdir(csrc) if re.fullmatch(r"kernels_\w+\.hip", f))
            folded = {m for f in all_ for m in re.findall(r'^#include "(kernels_\w+\.hip)"', open(os.path.join(csrc, f)).read(), re.M)}
            return [f for f in all_ if f not in folded and (lab or f not in B.LAB_SOURCES)]
        jobs = [(root, f) for root in (tmp, ROOT) for f in kernel_files(root)]
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            per_file = dict(zip(jobs, pool.map(lambda j: kernels(j[0], j[1], lab), jobs)))
    asm = {root: {n: (f, body) for (r, f), ks in per_file.items() if r == root for n, body in ks.items()} for root in (tmp, ROOT)}   # kernel symbol -> (file, lines)
    names = sorted({n for ks in asm.values() for n in ks}, key=lambda n: (asm[ROOT].get(n) or asm[tmp][n])[0] + n)
    pretty = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    rev_id = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    out = ["# gfx950 assembly of the working tree against %s (`tests/tools/asm_identity_folds.py %s%s`, source id %s)" % (rev_id, rev, " --lab" if lab else "", B.source_id(("-DVPT_LAB=%d" % lab,))), "",
           "`hipcc -S --cuda-device-only` with the product's flags, `-DVPT_LAB=%d`, no line tables.  identical: the same lines.  relabelled: the same lines but for the function's number in local labels and the next function's opening directives.  renamed: the same opcodes with other register numbers, the same register, scratch, occupancy and LDS figures." % lab, "",
           "| file | kernel | verdict | first differing line (revision / working tree) |", "|---|---|---|---|"]
    count = {"identical": 0, "relabelled": 0, "renamed": 0, "differs": 0}
    for n in names:
        (fo, old), (fn, new) = asm[tmp].get(n, (None, None)), asm[ROOT].get(n, (None, None))
        verdict, first = classify(old, new)
        count[verdict] += 1
        f = fn if fo in (None, fn) else (fo if fn is None else "%s -> %s" % (fo, fn))
        out.append("| %s | `%s` | %s | %s |" % (f, re.sub(r"^void |\(.*", "", pretty[n].replace("vpt::", "").replace("(anonymous namespace)::", "")), verdict, first.replace("|", "\\|")))
    out += ["", "%d kernels: %d identical, %d relabelled, %d renamed, %d differ." % (len(names), count["identical"], count["relabelled"], count["renamed"], count["differs"])]
    text = "\n".join(out) + "\n"
    if "--md" in sys.argv:
        open(os.path.join(ROOT, sys.argv[sys.argv.index("--md") + 1]), "w").write(text)
    print(text)
    sys.exit(1 if count["differs"] else 0)
