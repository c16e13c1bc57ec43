"""The gfx950 code objects inside a HIP shared library, and an ISA census of them.

A HIP .so keeps every translation unit's device code as a clang offload bundle in its
.hip_fatbin section (one bundle per TU, concatenated).  This reads the bundles, disassembles each
gfx950 code object with llvm-objdump and counts, per kernel symbol, the instruction classes the
build rules of DESIGN.md §4.9 forbid in shipped code:
  pk_f32 : packed-FP32 VALU (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32)
  calls  : s_swappc_b64 (a function call inside a kernel: nothing should be left un-inlined)
usage: python tools/codeobj.py LIB.so   -> one line per kernel with non-zero counts, then totals

python tools/codeobj.py --compare A B [--allow SYMBOL]... compares two builds (.so, .o or executables
with a .hip_fatbin section) byte for byte: the gfx950 code objects are paired by their kernel symbol
sets; a pair with the same bytes prints `identical`, any other prints every function symbol and
every <kernel>.kd descriptor whose bytes differ.  Exit status 0 only when everything matches or
every differing symbol is one given with --allow (a kernel's plain name, or the mangled symbol).
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def fatbin_section(path):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + out,
                               path, os.path.join(d, "copy")])
        return open(out, "rb").read()


def code_objects(blob, arch="gfx950"):
    """Every code object for `arch` in the concatenated bundles of a .hip_fatbin section."""
    objs = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.endswith(arch) and size:
                objs.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return objs


PATTERNS = {"pk_f32": re.compile(r"^\s*v_pk_(fma|mul|add)_f32\b"), "calls": re.compile(r"^\s*s_swappc_b64\b")}


def census(path, arch="gfx950"):
    """{kernel symbol: {class: count}} over every code object of the library."""
    out = {}
    for i, obj in enumerate(code_objects(fatbin_section(path), arch)):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f.name],
                                 capture_output=True, text=True, check=True).stdout
        sym = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                sym = m.group(1)
                out.setdefault(sym, {k: 0 for k in PATTERNS})
                continue
            if sym is None:
                continue
            for k, rx in PATTERNS.items():
                if rx.match(line):
                    out[sym][k] += 1
    return out


def _readelf(path, flag):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), flag, "--wide", path], capture_output=True, text=True,
                          check=True).stdout


def symbols(obj):
    """{name: bytes} of every function symbol and every kernel descriptor (<kernel>.kd) of one code
    object, cut out of it at the offsets llvm-readelf gives."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        sec = {}  # section index -> (address, file offset)
        for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+(?:PROGBITS)\s+([0-9a-f]+)\s+([0-9a-f]+)", _readelf(f.name, "-S"), re.M):
            sec[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
        out = {}
        for line in _readelf(f.name, "-s").splitlines():
            w = line.split()
            if len(w) != 8 or not w[6].isdigit() or int(w[6]) not in sec:
                continue
            if w[3] == "FUNC" or (w[3] == "OBJECT" and w[7].endswith(".kd")):
                addr, off = sec[int(w[6])]
                at = off + int(w[1], 16) - addr
                out[w[7]] = obj[at:at + int(w[2])]
        return out


def _allowed(sym, allow):
    name = sym[:-3] if sym.endswith(".kd") else sym
    return any(name == a or name.startswith("_Z%d%s" % (len(a), a)) for a in allow)


def compare(path_a, path_b, allow=(), out=sys.stdout):
    """Prints the comparison; returns (ok, the function symbols seen in A)."""
    sides = []
    for path in (path_a, path_b):
        groups = {}  # kernel symbol set -> [(object bytes, symbols)] in file order
        for obj in code_objects(fatbin_section(path)):
            sy = symbols(obj)
            groups.setdefault(frozenset(k[:-3] for k in sy if k.endswith(".kd")), []).append((obj, sy))
        sides.append(groups)
    ok = True
    seen = set()
    for key in sorted(set(sides[0]) | set(sides[1]), key=sorted):
        la, lb = sides[0].get(key, []), sides[1].get(key, [])
        label = "%d kernels, first %s" % (len(key), min(key)[:60] if key else "-")
        if len(la) != len(lb):
            ok = False
            print("object [%s]: %d in A, %d in B" % (label, len(la), len(lb)), file=out)
        for (oa, sa), (ob, sb) in zip(la, lb):
            seen |= {k for k in sa if not k.endswith(".kd")}
            if oa == ob:
                print("object [%s]: identical (%d bytes)" % (label, len(oa)), file=out)
                continue
            diff = sorted(k for k in set(sa) | set(sb) if sa.get(k) != sb.get(k))
            print("object [%s]: %d and %d bytes, %d of %d symbols differ" % (label, len(oa), len(ob), len(diff), len(set(sa) | set(sb))),
                  file=out)
            for k in diff:
                good = _allowed(k, allow)
                ok &= good
                print("  differs%s: %s" % (" (allowed)" if good else "", k), file=out)
            if not diff:  # the same code and descriptors: data, notes or symbol names differ
                ok = False
                print("  differs outside the function symbols and kernel descriptors", file=out)
    return ok, seen


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        rest = sys.argv[2:]
        allow = [rest[i + 1] for i, a in enumerate(rest) if a == "--allow"]
        paths = [a for i, a in enumerate(rest) if a != "--allow" and (i == 0 or rest[i - 1] != "--allow")]
        sys.exit(0 if compare(paths[0], paths[1], allow)[0] else 1)
    c = census(sys.argv[1])
    tot = {k: 0 for k in PATTERNS}
    for sym, cnt in sorted(c.items()):
        for k in tot:
            tot[k] += cnt[k]
        if any(cnt.values()):
            print("%-90s %s" % (sym[:90], " ".join("%s=%d" % kv for kv in cnt.items())))
    print("symbols %d  totals %s" % (len(c), " ".join("%s=%d" % kv for kv in tot.items())))
