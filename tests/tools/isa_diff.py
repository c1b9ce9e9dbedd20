"""Machine-code identity of the HIP kernels against a git revision: compiles every csrc/*.hip of REV (exported to a temporary
directory) and of the working tree to device-only gfx950 assembly with the flags of _build.py (FLAGS + the per-file EXTRA_FLAGS)
and compares them kernel by kernel - the body (instructions and labels), the .amdhsa_* descriptor and the metadata entry (VGPR /
AGPR / SGPR counts, LDS bytes, scratch, spills, arguments).  Comments, .file, .ident and the __hip_cuid_* symbol (a hash of the
source text) are ignored.  Prints one line per file and names every kernel that differs or exists on one side only; exit status
1 in that case.  Shows, without a GPU, that a source-level clean-up changed no kernel.
Usage: python tests/tools/isa_diff.py REV [file.hip ...]"""
import importlib, io, os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
b = importlib.import_module("subspace-multimodal-learning_amd._build")


def assembly(csrc, src, out):
    include = os.path.join(csrc, os.path.relpath(b.INCLUDE, b.CSRC))      # include/smml.h of the same tree
    if not os.path.exists(os.path.join(csrc, src)):
        return ""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *b.FLAGS, *b.EXTRA_FLAGS.get(src, []), "-I", csrc, "-I", include, "-S", "--cuda-device-only",
           os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {os.path.join(csrc, src)}:\n{r.stderr}")
    return open(out).read()


def clean(text):
    lines = (l.split(";")[0].strip() for l in text.split("\n"))          # ';' starts a comment; no operand of these files holds one
    return [l for l in lines if l and not l.startswith((".file", ".ident")) and "__hip_cuid_" not in l]


def kernels(txt):
    """name -> cleaned lines of the kernel's body with its .amdhsa_kernel descriptor, then of its metadata entry"""
    ks = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n", txt, re.M):
        start = re.search(rf"^{re.escape(m.group(1))}:", txt, re.M).start()
        ks[m.group(1)] = clean(txt[start:txt.index(".end_amdhsa_kernel", m.end())])
    meta = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", txt, re.S | re.M)
    for entry in re.split(r"^  - ", meta.group(1) if meta else "", flags=re.M)[1:]:
        ks[re.search(r"^\s+\.name:\s+(\S+)", entry, re.M).group(1)] += ["<metadata>"] + clean(entry)
    return ks


if __name__ == "__main__":
    rev = sys.argv[1]
    csrc_rel = os.path.relpath(b.CSRC, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, csrc_rel, os.path.relpath(b.INCLUDE, ROOT)], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        old_csrc = os.path.join(tmp, csrc_rel)
        srcs = sys.argv[2:] or sorted(set(b.sources()) | {f for f in os.listdir(old_csrc) if f.endswith(".hip")})
        jobs = [(c, s, os.path.join(tmp, f"{tag}_{s[:-4]}.s")) for s in srcs for tag, c in (("old", old_csrc), ("new", b.CSRC))]
        with ThreadPoolExecutor(max_workers=16) as ex:
            asm = list(ex.map(lambda j: kernels(assembly(*j)), jobs))
    full = subprocess.run(["git", "-C", ROOT, "rev-parse", rev], capture_output=True, text=True).stdout.strip()
    print(f"# gfx950 kernels of the working tree against {rev} = {full}: {' '.join(b.FLAGS)}; {b.EXTRA_FLAGS}")
    differ = False
    for i, src in enumerate(srcs):
        old, new = asm[2 * i], asm[2 * i + 1]
        bad = [f"only in {rev}: {k}" for k in sorted(set(old) - set(new))] + [f"only in the working tree: {k}" for k in sorted(set(new) - set(old))]
        bad += [f"differs: {k}" for k in sorted(set(old) & set(new)) if old[k] != new[k]]
        print(f"{src}: {len(old)} kernels at {rev}, {len(new)} in the working tree, {sum(old[k] == new.get(k) for k in old)} identical")
        for x in bad:
            print("   ", x)
        differ |= bool(bad)
    sys.exit(1 if differ else 0)
