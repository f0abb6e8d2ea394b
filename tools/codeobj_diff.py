#!/usr/bin/env python3
"""Is the device code of two builds the same?  Compares the gfx950 code objects embedded in the objects of two build
directories (make OUT=...): unit by unit byte for byte, and -- for kernels that moved from one unit to another -- kernel by
kernel (disassembly with addresses relative to the kernel's start and pc-relative addresses of data objects by the object's name, and
the register / LDS / scratch figures of the metadata).

    python tools/codeobj_diff.py OLD_OBJ_DIR NEW_OBJ_DIR [--moved old_unit:new_unit ...]

Prints a table of unit or kernel against identical / differs / no kernels; exit status 1 when anything differs.
Build both trees in the SAME directory with the same OUT, one after the other (move the first build's obj/ away): the toolchain's
per-unit id depends on the path and the command line and goes into the code object, so builds at two paths differ byte for byte
in every unit that has a kernel.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp):
    """The gfx950 code object of an object file (bytes; b'' when it carries none)."""
    fat, co = os.path.join(tmp, os.path.basename(obj) + ".fat"), os.path.join(tmp, os.path.basename(obj) + ".co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "x.o")], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return b"", None
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}"],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
        return b"", None
    return open(co, "rb").read(), co


def kernels(co):
    """{kernel name: (normalised disassembly, resource tuple)} of one code object."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for k in notes.split("  - .agpr_count")[1:]:
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        res[re.search(r"\.name:\s+(\S+)", k).group(1)] = (g("vgpr_count"), int(re.match(r":\s+(\d+)", k).group(1)), g("sgpr_count"),
                                                           g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    syms = []  # (address, size, name) of the data objects a kernel can point at
    for line in subprocess.run([f"{LLVM}/llvm-objdump", "-t", co], capture_output=True, text=True, check=True).stdout.split("\n"):
        m = re.match(r"^([0-9a-f]+)\s.*\sO\s+\S+\s+([0-9a-f]+)\s+(\S+)$", line)
        if m:
            syms.append((int(m.group(1), 16), int(m.group(2), 16), m.group(3)))
    for line in subprocess.run([f"{LLVM}/llvm-readelf", "-r", co], capture_output=True, text=True, check=True).stdout.split("\n"):
        m = re.match(r"^([0-9a-f]+)\s+[0-9a-f]+\s+R_AMDGPU_ABS64\s+[0-9a-f]+\s+(\S+) \+ (\d+)$", line)
        if m:  # a GOT entry: the address of a data object, filled in at load time
            syms.append((int(m.group(1), 16), 8, "got:%s+%s" % (m.group(2), m.group(3))))

    def pc_relative(line, prev):
        """`s_getpc_b64 s[n:..]` then `s_add_u32 sn, sn, literal` is the address of a data object outside the kernel, relative to
        the s_add_u32: it moves whenever a kernel between the two changes size.  The literal becomes the object's name + offset."""
        g, a = re.match(r"s_getpc_b64 s\[(\d+):", prev), re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+)\s+//\s*([0-9A-Fa-f]{8,}):", line)
        if not (g and a and g.group(1) == a.group(1) == a.group(2)):
            return line
        target = int(a.group(4), 16) + int(a.group(3), 16)
        for addr, size, sym in syms:
            if addr <= target < addr + max(size, 1):
                return "s_add_u32 s%s, s%s, <%s+%d>  // %s:" % (a.group(1), a.group(1), sym, target - addr, a.group(4))
        return line

    out, name, base, body, prev = {}, None, 0, [], ""
    for line in dis.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            if name in res:
                out[name] = ("\n".join(body), res[name])
            name, base, body = m.group(2), int(m.group(1), 16), []
            continue
        if name is None:
            continue
        line, prev = pc_relative(line.strip(), prev), line.strip()
        # addresses (the trailing "// 000000001234:" and branch targets "<sym+0x..>") relative to the kernel's start
        line = re.sub(r"//\s*([0-9A-Fa-f]{8,}):", lambda a: "// +%x:" % (int(a.group(1), 16) - base), line)
        body.append(line.strip())
    if name in res:
        out[name] = ("\n".join(body), res[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--moved", nargs="*", default=[], help="old_unit:new_unit whose kernels are compared one by one")
    a = ap.parse_args()
    bad = 0
    moved = dict(m.split(":") for m in a.moved)
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        units = sorted(f[:-2] for f in os.listdir(a.new) if f.endswith(".o"))
        print(f"{'unit / kernel':100s} result")
        for u in units:
            new, new_co = code_object(os.path.join(a.new, u + ".o"), t_new)
            if u in moved or u in moved.values():
                continue
            old_path = os.path.join(a.old, u + ".o")
            if os.path.exists(old_path):
                old, _ = code_object(old_path, t_old)
                same = old == new
                print(f"{u + '.o  code object, ' + str(len(new)) + ' bytes, sha256 ' + hashlib.sha256(new).hexdigest()[:16]:100s} {'identical' if same else 'DIFFERS'}")
                bad += not same
            else:
                ks = kernels(new_co) if new_co else {}
                print(f"{u + '.o  (new unit)':100s} {'no kernels' if not ks else 'DIFFERS: %d kernels' % len(ks)}")
                bad += bool(ks)
        for o, n in moved.items():
            _, oco = code_object(os.path.join(a.old, o + ".o"), t_old)
            _, nco = code_object(os.path.join(a.new, n + ".o"), t_new)
            ok, nk = kernels(oco), kernels(nco)
            for name in sorted(set(ok) | set(nk)):
                if name not in ok or name not in nk:
                    res = "DIFFERS: only in " + (o if name in ok else n)
                else:
                    res = "identical" if ok[name] == nk[name] else ("DIFFERS: " + ("resources" if ok[name][1] != nk[name][1] else "disassembly"))
                if name in nk:
                    v = nk[name][1]
                    res += "  (vgpr %d agpr %d sgpr %d scratch %d lds %d)" % v
                print(f"{o + '.o -> ' + n + '.o  ' + name:100s} {res}")
                bad += res.startswith("DIFFERS")
            if os.path.exists(os.path.join(a.new, o + ".o")):  # the unit the kernels left
                _, lco = code_object(os.path.join(a.new, o + ".o"), t_new)
                left = kernels(lco) if lco else {}
                print(f"{o + '.o  (this tree)':100s} {'no kernels' if not left else 'DIFFERS: %d kernels' % len(left)}")
                bad += bool(left)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
