#!/usr/bin/env python3
"""One line per kernel of a translation unit: a SHA-1 of its gfx950 function body and its resource figures, from
`hipcc -S --cuda-device-only` of the source with the library's flags.  Run it before and after a change that must leave existing
kernels alone and compare the lines (local labels are renumbered per file, so they are stripped with the comments before
hashing).  No GPU needed.

    python tools/core_instantiations.py [out.txt]                                  the instantiations of core_fused_kernel (km_core.hip)
    python tools/core_instantiations.py --source km_generic.hip [--prefix P] [out.txt]
                                                                                   every __global__ symbol of the unit (whose mangled
                                                                                   name starts with P), by mangled name
    python tools/core_instantiations.py --csrc DIR ...                             the sources of another checkout (its koemorph_amd/csrc)
"""
import argparse, hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import build

ap = argparse.ArgumentParser()
ap.add_argument("--source")
ap.add_argument("--prefix", default="")
ap.add_argument("--csrc", default=build.CSRC)
ap.add_argument("out", nargs="?")
args = ap.parse_args()
fused = args.source is None          # the original report: core_fused_kernel by template arguments
prefix = "_ZN2km17core_fused_kernel" if fused else args.prefix

src = os.path.join(args.csrc, args.source or "km_core.hip")
flags = [f for f in build._flags() if f != "-I" + build.CSRC] + ["-I" + args.csrc]
with tempfile.TemporaryDirectory() as tmp:
    asm = os.path.join(tmp, "unit.s")
    subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
rows = {}
for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
    if m.group(1) in kernels and m.group(1).startswith(prefix):
        body = re.sub(r";.*", "", re.sub(r"\.L\w+", "L", m.group(2)))
        rows[m.group(1)] = [hashlib.sha1(body.encode()).hexdigest()[:16], str(len(body.splitlines()))]
for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk)
    if name and name.group(1) in rows:
        rows[name.group(1)] += [re.search(r"\.%s:\s+(\d+)" % k, blk).group(1) for k in
                                ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                 "kernarg_segment_size")]
what = "instantiation <ATTN, FUSE_DB, NP, TAB>" if fused else "kernel of %s" % args.source
lines = [what + " | sha1(body) | lines | vgpr | sgpr | vgpr spills | static lds | scratch | kernarg"]
for name in sorted(rows):
    label = "<%s, %s, %s, %s>" % re.search(r"ILb(\d)ELb(\d)ELi(\d)ELb(\d)E", name).groups() if fused else name
    lines.append(label + " | " + " | ".join(rows[name]))
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
