#!/usr/bin/env python3
r"""Compare the kernels of two device builds of a .hip file: isa_diff.py [--key REGEX] OLD.elf NEW.elf [OLD.s NEW.s]

The ELFs come from build.sh's flags plus `--cuda-device-only --no-gpu-bundle-output -c` (one sized FUNC symbol per kernel,
no relocations: a symbol's bytes are position-independent), the optional .s files from the same flags with -S.  Per kernel
present in both it compares the raw instruction bytes of the symbol's range in .text and, with the .s files, its
.amdhsa_* directive block (registers, LDS, scratch, kernarg size, preload).  Bytes, not -S text: .LBB<n>_<m> labels carry
the function's ordinal and shift when a kernel is removed.  Exit status 1 if any common kernel differs.

--key REGEX: a kernel whose mangled name matches is known by the regex's groups instead (a group that did not take part counts as 0),
so that a template that gained a parameter is still compared with what it was: with
--key 'multi_query_decode_kernelILi(\d+)ELi(\d+)ELb([01])E(?:Lb([01])E)?' the instantiation <128, 2, true> of the old build meets
<128, 2, true, false> of the new one, and <.., true> is reported as added.
"""
import os
import re
import shutil
import subprocess
import sys

_ROCM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
READELF = shutil.which("llvm-readelf") or (_ROCM if os.path.exists(_ROCM) else "readelf")


KEY = None


def known_as(name):
    m = KEY.search(name) if KEY else None
    return name if not m else name[m.start():m.start(1)] + " <" + ", ".join(g or "0" for g in m.groups()) + ">"


def kernels(elf):
    """{name: instruction bytes} of every FUNC symbol in .text."""
    sec = subprocess.check_output([READELF, "-S", "-W", elf], text=True)
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    if not m:
        sys.exit(f"isa_diff.py: no .text section header found in the output of `{READELF} -S -W {elf}`")
    addr, off, size = (int(x, 16) for x in m.groups())
    idx = re.search(r"\[\s*(\d+)\]\s+\.text\s", sec).group(1)
    text = open(elf, "rb").read()[off:off + size]
    out = {}
    for line in subprocess.check_output([READELF, "-s", "-W", elf], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] == idx:
            a, n = int(f[1], 16) - addr, int(f[2])
            out[known_as(f[7])] = text[a:a + n]
    return out


def directives(asm):
    """{name: sorted .amdhsa_* lines} from a -S build."""
    out, cur = {}, None
    for line in open(asm):
        s = line.split()
        if len(s) == 2 and s[0] == ".amdhsa_kernel":
            cur = out.setdefault(known_as(s[1]), [])
        elif s and s[0] == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s and s[0].startswith(".amdhsa_"):
            cur.append(" ".join(s))
    return out


def main():
    global KEY
    if len(sys.argv) > 2 and sys.argv[1] == "--key":
        KEY = re.compile(sys.argv[2])
        del sys.argv[1:3]
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dold, dnew = (directives(sys.argv[3]), directives(sys.argv[4])) if len(sys.argv) > 4 else ({}, {})
    common = sorted(set(old) & set(new))
    differ = []
    for k in common:
        why = []
        if old[k] != new[k]:
            why.append(f"instruction bytes ({len(old[k])} -> {len(new[k])})")
        if dold.get(k) != dnew.get(k):
            why += sorted(set(dnew.get(k, [])) ^ set(dold.get(k, [])))
        if why:
            differ.append((k, why))
    for k in sorted(set(old) - set(new)):
        print("gone  ", k)
    for k in sorted(set(new) - set(old)):
        print("added ", k)
    for k, why in differ:
        print("DIFFER", k, "::", "; ".join(why))
    print(f"{len(old)} -> {len(new)} kernels: {len(common)} in common, {len(old) - len(common)} gone, "
          f"{len(new) - len(common)} added, {len(differ)} of the common ones differ"
          f"{'' if dold else ' (instruction bytes only: no .s files given)'}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
