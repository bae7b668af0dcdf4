"""Per-kernel digest of the gfx950 code in the objects of a build, and a comparison of two such listings.

A refactor of the kernel sources must not move an instruction of a kernel it does not mean to change.  This prints, for
every kernel of every object under ir2rgb_amd/lib/obj (or of the objects named), one tab-separated line:

    object  instructions  sha1 of the disassembly (addresses and symbol names removed)  VGPRs  SGPRs  LDS bytes
    private-segment bytes  MFMA / LDS read / LDS-DMA / s_barrier / s_waitcnt counts  demangled name

and compares two listings kernel by kernel (paired by demangled name):

    python tools/kernel_digest.py > new.tsv
    python tools/kernel_digest.py --diff old.tsv new.tsv [--map REGEX=REPLACEMENT ...]

--map rewrites the OLD names before pairing (re.sub, applied in the order given): the explicit table of kernels that were
renamed or lost a template parameter.  Exit status of --diff: 1 if a paired kernel changed or one exists only in NEW.
CPU only (hipcc cross-compiles; the code objects are read with llvm-objdump / llvm-readelf).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_lds_war import LLVM, ROOT, device_asm  # noqa: E402

LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
COLUMNS = ("object", "insts", "sha1", "vgpr", "sgpr", "lds", "private", "mfma", "ds_read", "lds_dma", "barrier", "waitcnt", "name")


def kernel_meta(co):
    """{mangled name: (vgpr, sgpr, lds, private)} from the code object's metadata note."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        f = {k: v for k, v in re.findall(r"^\s+\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)$",
                                         block, re.M)}
        meta[f["name"]] = (f["vgpr_count"], f["sgpr_count"], f["group_segment_fixed_size"], f["private_segment_fixed_size"])
    return meta


def demangle(names):
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", check=True, capture_output=True, text=True).stdout
    return out.splitlines()


def digest(obj, tmp):
    """-> rows (as in COLUMNS) for the kernels of one host object."""
    lines = device_asm(obj, tmp)
    if not lines:
        return []
    meta = kernel_meta(os.path.join(tmp, os.path.basename(obj)) + ".co")
    bodies, cur = {}, None
    for line in lines:
        m = LABEL.match(line)
        if m:
            cur = bodies.setdefault(m.group(1), [])
            continue
        s = line.split("//")[0].strip()
        if cur is not None and s and not s.startswith("Disassembly"):
            cur.append(" ".join(s.split()))
    names = [n for n in bodies if n in meta]
    rows = []
    for name, pretty in zip(names, demangle(names)):
        body = bodies[name]
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):   # padding behind s_endpgm ("...": objdump's run of zero bytes)
            body.pop()
        ops = [i.split()[0] for i in body]
        n = lambda pred: sum(1 for i, o in zip(body, ops) if pred(i, o))  # noqa: E731
        rows.append((os.path.basename(obj), len(body), hashlib.sha1("\n".join(body).encode()).hexdigest()[:16], *meta[name],
                     n(lambda i, o: o.startswith("v_mfma")), n(lambda i, o: o.startswith(("ds_read", "ds_load"))),
                     n(lambda i, o: o.startswith(("buffer_load", "global_load")) and i.endswith("lds")),
                     n(lambda i, o: o == "s_barrier"), n(lambda i, o: o == "s_waitcnt"), pretty))
    return rows


def listing(paths):
    if not paths:
        objdir = os.path.join(ROOT, "ir2rgb_amd", "lib", "obj")
        paths = sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o"))
    print("#" + "\t".join(COLUMNS))
    total = insts = 0
    with tempfile.TemporaryDirectory(prefix="kdigest") as tmp:
        for p in paths:
            for row in sorted(digest(p, tmp), key=lambda r: r[-1]):
                print("\t".join(str(c) for c in row))
                total += 1
                insts += row[1]
    print(f"# {total} kernels, {insts} instructions")
    return 0


def read_listing(path):
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\n").split("\t")
        rows[f[-1]] = dict(zip(COLUMNS, f))
    return rows


def diff(old_path, new_path, maps):
    old, new = {}, read_listing(new_path)
    for name, row in read_listing(old_path).items():
        for pat, repl in maps:
            name = re.sub(pat, repl, name)
        if name in old:
            raise SystemExit(f"--map sends two old kernels to {name}")
        old[name] = row
    same, changed = [], []
    for name in sorted(set(old) & set(new)):
        o, n = old[name], new[name]
        (same if all(o[c] == n[c] for c in COLUMNS[1:-1]) else changed).append(name)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"identical: {len(same)}")
    print(f"changed: {len(changed)}")
    for name in changed:
        o, n = old[name], new[name]
        print("   ", name[:160])
        print("        " + ", ".join(f"{c} {o[c]} -> {n[c]}" if o[c] != n[c] else f"{c} {o[c]}" for c in COLUMNS[1:-1] if c != "sha1"))
    for title, names, rows in (("only-old", only_old, old), ("only-new", only_new, new)):
        print(f"{title}: {len(names)}" + (f" ({sum(int(rows[k]['insts']) for k in names)} instructions)" if names else ""))
        for name in names:
            print("   ", rows[name]["object"], name[:160])
    return 1 if changed or only_new else 0


def main(argv):
    if argv and argv[0] == "--diff":
        maps = []
        rest = argv[3:]
        while rest:
            if rest[0] != "--map" or len(rest) < 2 or "=" not in rest[1]:
                raise SystemExit(__doc__)
            maps.append(tuple(rest[1].split("=", 1)))
            rest = rest[2:]
        return diff(argv[1], argv[2], maps)
    return listing(argv)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
