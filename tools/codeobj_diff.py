#!/usr/bin/env python3
"""Compare the gfx950 code objects of two libsng.so builds (a refactor's proof that the device code is unchanged):

  tools/codeobj_diff.py <parent libsng.so> <this libsng.so>

A byte-identical code object is reported as such.  Otherwise, per kernel symbol: the disassembly with its
addresses and encodings stripped, and the kernel's entry in the AMDHSA metadata note.  Symbols that only one build
has are listed (a feature adds kernels; a removed one fails), and the symbols both have are compared all the same.
Prints "N kernels, D differ" and exits 1 when D > 0 or the parent has a symbol this build lacks."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True, cwd=cwd).stdout


def code_object(lib, workdir):
    copy = shutil.copy(lib, workdir)   # the code object is written beside the library
    run("llvm-objdump", "--offloading", copy, cwd=workdir)
    objs = [f for f in os.listdir(workdir) if "amdgcn-amd-amdhsa--gfx950" in f]
    assert len(objs) == 1, f"{lib}: {len(objs)} gfx950 code objects"
    return os.path.join(workdir, objs[0])


def functions(co):
    """symbol -> its instructions, without the `// address: encoding` tail and without the pc-relative distance
    of a call (the s_add_u32 literal behind s_getpc_b64), which is an address like those."""
    out, cur = {}, None
    for line in run("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":   # "...": the padding up to the next symbol
            ins = line.split("//")[0].strip()
            if cur and cur[-1].startswith("s_getpc_b64"):
                ins = re.sub(r"0x[0-9a-f]+$", "<rel>", ins)
            cur.append(ins)
    return out


def metadata(co):
    """kernel name -> its entry of amdhsa.kernels, as text."""
    notes = run("llvm-readelf", "--notes", co).splitlines()
    start = next(i for i, line in enumerate(notes) if line.strip() == "amdhsa.kernels:")
    out, cur = {}, []
    for line in notes[start + 1:]:
        if not line.startswith("  "):
            break
        if line.startswith("  - "):
            cur = []
        cur.append(line)
        m = re.match(r"^\s+\.name:\s+(\S+)$", line)
        if m and line.startswith("    .name:"):
            out[m.group(1)] = cur
    return out


def main(a, b):
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        ca, cb = code_object(a, da), code_object(b, db)
        with open(ca, "rb") as fa, open(cb, "rb") as fb:
            same = fa.read() == fb.read()
        fa, fb, ma, mb = functions(ca), functions(cb), metadata(ca), metadata(cb)
    removed, added = sorted((set(fa) | set(ma)) - (set(fb) | set(mb))), sorted((set(fb) | set(mb)) - (set(fa) | set(ma)))
    for k in removed:
        print("  only in the parent:", k)
    for k in added:
        print("  only in this build:", k)
    shared = sorted(set(fa) & set(fb))
    differ = [k for k in shared if fa[k] != fb[k] or ma.get(k) != mb.get(k)]
    print(f"{len(set(ma) & set(mb))} kernels ({len(shared)} symbols) in both, {len(differ)} differ in disassembly or "
          f"AMDHSA metadata; {len(added)} added, {len(removed)} removed" + ("; code objects byte-identical" if same else ""))
    for k in differ:
        print("  differs:", k)
    return 1 if differ or removed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
