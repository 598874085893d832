"""Does the working tree compile to the same kernels as a git revision?  The check of a refactor (not a pytest; needs hipcc only, no GPU): every kernels_*.hip
of the revision (its csrc/ and include/ exported with git archive) and of the working tree is compiled to gfx950 assembly with the product's flags
(tests/tools/spill_report.py's compile line without line tables: source line numbers move in a refactor), and every kernel symbol is classified as
  identical  the same lines (lines that name the per-file __hip_cuid_ symbol are dropped);
  renamed    the same sequence of opcodes once every register operand is replaced by its class (v, s, a; vcc / exec as they are), and the same NumVgprs,
             TotalNumSgprs, ScratchSize, Occupancy and LDS size;
  differs    anything else, with the first differing line.
Exit status 1 if any kernel differs.
    python tests/tools/asm_identity.py <git-rev> [--lab] [--md profiles/NAME.md]"""
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
    return {n: lines[i:j] for (i, n), (j, _) in zip(starts, starts[1:] + [(len(lines), "")])}


def shape(body):
    """A kernel's opcodes with every register operand reduced to its class, and its resource figures."""
    ops = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", l.split(";")[0]).split() for l in body if re.match(r"^\s+[a-z]\w*\s", l + " ")]
    return ops, [l.strip() for l in body if l.strip().startswith(FIGURES)]


def classify(old, new):
    if old is None or new is None:
        return "differs", "only in the %s" % ("working tree" if old is None else "revision")
    if old == new:
        return "identical", ""
    first = next(("`%s` / `%s`" % (a.strip(), b.strip()) for a, b in zip(old, new) if a != b), "%d / %d lines" % (len(old), len(new)))
    return ("renamed" if shape(old) == shape(new) else "differs"), first


if __name__ == "__main__":
    rev, lab = sys.argv[1], int("--lab" in sys.argv)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, PKG + "/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        kernel_files = lambda root: sorted(f for f in os.listdir(os.path.join(root, PKG, "csrc")) if re.fullmatch(r"kernels_\w+\.hip", f) and (lab or f not in B.LAB_SOURCES))
        jobs = [(root, f) for root in (tmp, ROOT) for f in kernel_files(root)]
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            asm = dict(zip(jobs, pool.map(lambda j: kernels(j[0], j[1], lab), jobs)))
    names = sorted({(f, n) for (_, f), ks in asm.items() for n in ks})
    pretty = dict(zip([n for _, n in names], subprocess.run(["c++filt"], input="\n".join(n for _, n in names), capture_output=True, text=True).stdout.split("\n")))
    rev_id = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    out = ["# gfx950 assembly of the working tree against %s (`tests/tools/asm_identity.py %s%s`, source id %s)" % (rev_id, rev, " --lab" if lab else "", B.source_id(("-DVPT_LAB=%d" % lab,))), "",
           "`hipcc -S --cuda-device-only` with the product's flags, `-DVPT_LAB=%d`, no line tables.  identical: the same lines.  renamed: the same opcodes with other register numbers, the same register, scratch, occupancy and LDS figures." % lab, "",
           "| file | kernel | verdict | first differing line (revision / working tree) |", "|---|---|---|---|"]
    count = {"identical": 0, "renamed": 0, "differs": 0}
    for f, n in names:
        verdict, first = classify(asm.get((tmp, f), {}).get(n), asm.get((ROOT, f), {}).get(n))
        count[verdict] += 1
        out.append("| %s | `%s` | %s | %s |" % (f, re.sub(r"^void |\(.*", "", pretty[n].replace("vpt::", "").replace("(anonymous namespace)::", "")), verdict, first.replace("|", "\\|")))
    out += ["", "%d kernels: %d identical, %d renamed, %d differ." % (len(names), count["identical"], count["renamed"], count["differs"])]
    text = "\n".join(out) + "\n"
    if "--md" in sys.argv:
        open(os.path.join(ROOT, sys.argv[sys.argv.index("--md") + 1]), "w").write(text)
    print(text)
    sys.exit(1 if count["differs"] else 0)
