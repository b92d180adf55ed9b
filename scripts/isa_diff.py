#!/usr/bin/env python3
"""isa_diff.py <old.s> <new.s>: compare two `hipcc -S --cuda-device-only` listings function by function (no GPU).

Comments, blank lines and the `.ident` line are dropped and the local labels of a function renumbered in order of appearance;
what is left of a function - instructions, its `.amdhsa_kernel` block and its entry in the metadata (VGPR / SGPR / scratch /
LDS figures) - must be the same text.  Prints `identical`, `DIFFERENT`, `absent` (only in <old.s>) or `new` per function and
exits 1 unless every function both listings define is identical."""
import re
import sys


def functions(path):
    out, name = {}, None
    for line in open(path):
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", line.split(";")[0].rstrip())   # (a hash of the source text)
        m = re.match(r"^(\w+):$", line) or re.match(r"^    \.name:\s+(\w+)$", line)
        s = re.match(r"^\s+\.section\s+\.text\.(\w+),", line)
        if re.match(r"^  - \.", line) or ".amdgpu_metadata" in line or (s and s.group(1) != name):
            name = None   # the next function's header, or a new metadata entry: its .name line says whose
            pending = out.setdefault("", [])
            del pending[:]
        if m and not m.group(1).startswith("."):
            name = m.group(1) + (" (metadata)" if ".name:" in line else "")
            out[name] = out.pop("", []) if ".name:" in line else []
        if line.strip() and ".ident" not in line:
            out.setdefault(name or "", []).append(line)
    out.pop("", None)
    for body in out.values():   # local labels in order of appearance
        seen = {}
        body[:] = [re.sub(r"\.L\w+", lambda t: seen.setdefault(t.group(0), ".L%d" % len(seen)), l) for l in body]
    return out


old, new = functions(sys.argv[1]), functions(sys.argv[2])
bad = 0
for k in sorted(set(old) | set(new)):
    verdict = "absent" if k not in new else "new" if k not in old else "identical" if old[k] == new[k] else "DIFFERENT"
    bad += verdict == "DIFFERENT"
    print("%-10s %5d lines  %s" % (verdict, len(new.get(k, old.get(k))), k))
sys.exit(1 if bad else 0)
