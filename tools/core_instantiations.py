#!/usr/bin/env python3
"""One line per instantiation of core_fused_kernel: a SHA-1 of its gfx950 function body and its resource figures, from
`hipcc -S --cuda-device-only` of koemorph_amd/csrc/km_core.hip with the library's flags.  Run it before and after a change that
must leave existing instantiations alone and compare the lines (local labels are renumbered per file, so they are stripped with
the comments before hashing).  No GPU needed.

    python tools/core_instantiations.py [out.txt]
"""
import hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import build

src = os.path.join(build.CSRC, "km_core.hip")
with tempfile.TemporaryDirectory() as tmp:
    asm = os.path.join(tmp, "km_core.s")
    subprocess.run([build._hipcc()] + build._flags() + ["--cuda-device-only", "-S", src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
rows = {}
for m in re.finditer(r"^(_ZN2km17core_fused_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
    body = re.sub(r";.*", "", re.sub(r"\.L\w+", "L", m.group(2)))
    rows[m.group(1)] = [hashlib.sha1(body.encode()).hexdigest()[:16], str(len(body.splitlines()))]
for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk)
    if name and name.group(1) in rows:
        rows[name.group(1)] += [re.search(r"\.%s:\s+(\d+)" % k, blk).group(1) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                 "kernarg_segment_size")]
lines = ["instantiation <ATTN, FUSE_DB, NP, TAB> | sha1(body) | lines | vgpr | sgpr | vgpr spills | static lds | scratch | kernarg"]
for name in sorted(rows):
    t = re.search(r"ILb(\d)ELb(\d)ELi(\d)ELb(\d)E", name).groups()
    lines.append(f"<{t[0]}, {t[1]}, {t[2]}, {t[3]}> | " + " | ".join(rows[name]))
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
