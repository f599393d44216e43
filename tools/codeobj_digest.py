"""One line per gfx950 kernel of the library: name, a hash of its instructions, instruction count and resources (no GPU needed).

    python tools/codeobj_digest.py > profiles/rNN_codeobj_after.txt
    python tools/codeobj_digest.py --diff parent.txt after.txt        # the kernels whose line differs, and the names on one side only

Every .hip source is compiled with the product's flags to device assembly in a temporary directory outside the tree; only this
table is kept.  The hash covers a kernel's instruction text with comments and directives dropped and local labels renumbered in
order of appearance, so moving a kernel to another file (or to another place in its file) leaves it alone while any change of an
instruction, an operand or a register shows.  The resource columns are those of tools/kernel_resources.py.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import build as B  # noqa: E402

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def short_name(mangled):
    dem = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    dem = re.sub(r"\(anonymous namespace\)::", "", dem)
    dem = re.sub(r"^void ", "", dem)
    return re.sub(r"\((?:r2f::|[a-z]).*$", "", dem).replace("r2f::", "")


def kernel_texts(asm):
    """{mangled kernel name: [normalised instruction lines]} of one device assembly file."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, name, lines, labels = {}, None, [], {}
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        if name is None:
            if line.endswith(":") and line[:-1] in kernels:
                name, lines, labels = line[:-1], [], {}
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = lines
            name = None
            continue
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue  # blank, comment or directive
        lines.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), line))
    return out


def digest_source(src, tmp):
    out = os.path.join(tmp, src + ".s")
    cmd, rc, log = B._compile_one(B._hipcc(), src, out, ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    if rc:
        raise SystemExit(f"{cmd}\n{log}")
    res = {}
    for blk in re.split(r"remark: Function Name: ", log)[1:]:
        def g(key):
            m = re.search(re.escape(key) + r": (\d+)", blk)
            return int(m.group(1)) if m else -1
        res[blk.split()[0]] = (g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("ScratchSize [bytes/lane]"),
                               g("Occupancy [waves/SIMD]"), g("LDS Size [bytes/block]"))
    rows = []
    with open(out) as f:
        for mangled, lines in kernel_texts(f.read()).items():
            insts = [ln for ln in lines if not ln.endswith(":")]
            h = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
            rows.append((short_name(mangled), src, h, len(insts)) + res.get(mangled, (-1,) * 7))
    return rows


def table():
    hips = [s for s in B.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory(prefix="r2f_codeobj_") as tmp, ThreadPoolExecutor(len(hips)) as pool:
        rows = sorted(r for part in pool.map(lambda s: digest_source(s, tmp), hips) for r in part)
    print("# tools/codeobj_digest.py: hipcc --offload-arch=gfx950, the product's flags; hash = sha256[:16] of the kernel's instructions")
    print("# (comments and directives dropped, local labels renumbered); LDS = static only; waves/SIMD = register-limited occupancy")
    print(f"{'kernel':<60}{'file':<24}{'hash':<18}{'insts':>6}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'spilled':>8}{'scratch B':>10}{'waves/SIMD':>11}{'LDS':>7}")
    for r in rows:
        print(f"{r[0]:<60}{r[1]:<24}{r[2]:<18}{r[3]:>6}{r[4]:>5}{r[5]:>5}{r[6]:>5}{r[7]:>8}{r[8]:>10}{r[9]:>11}{r[10]:>7}")
    bad = [r for r in rows if r[7] > 0 or r[8] > 0]
    print(f"# {len(rows)} kernels; with spilled registers or scratch: {len(bad)}" + "".join(f"\n#   {r[0]}" for r in bad))


def diff(path_a, path_b):
    def load(p):
        with open(p) as f:
            rows = [ln for ln in f if ln.strip() and not ln.startswith("#") and not ln.startswith("kernel ")]
        # a name with template arguments holds blanks, and a file name as wide as its column runs into the hash: the file column is
        # the first word that ends in .hip
        out = {}
        for ln in rows:
            m = re.match(r"(.+?)\s+(\w+\.hip)\s*(.*)", ln)
            out[" ".join(m.group(1).split())] = [m.group(2)] + m.group(3).split()
        return out

    a, b = load(path_a), load(path_b)
    same = [k for k in a if k in b and a[k][1:] == b[k][1:]]
    moved = [k for k in same if a[k][0] != b[k][0]]
    print(f"# {path_a} ({len(a)} kernels) against {path_b} ({len(b)} kernels)")
    print(f"# identical hash and resources: {len(same)} kernels, {len(moved)} of them in another file")
    for k in sorted(moved):
        print(f"  moved      {k}: {a[k][0]} -> {b[k][0]}")
    cols = "file hash insts VGPR AGPR SGPR spilled scratch waves/SIMD LDS".split()
    for k in sorted(k for k in a if k in b and k not in same):
        print(f"  changed    {k}: " + ", ".join(f"{c} {x} -> {y}" for c, x, y in zip(cols, a[k], b[k]) if x != y))
    for k in sorted(set(a) - set(b)):
        print(f"  only in A  {k}: " + " ".join(a[k]))
    for k in sorted(set(b) - set(a)):
        print(f"  only in B  {k}: " + " ".join(b[k]))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        diff(sys.argv[2], sys.argv[3])
    else:
        table()
