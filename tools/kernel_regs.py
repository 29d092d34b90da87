#!/usr/bin/env python3
"""Register / scratch usage of every kernel of one HIP translation unit (from the code object metadata):
    python tools/kernel_regs.py sqlite-vector_amd/csrc/vg_multi.hip [--all | --digest] [-DNAME[=VALUE] ...]
prints name, VGPRs, spilled VGPRs, scratch bytes; without --all only kernels that spill or use scratch.
-D... arguments go to the compile: the batch units exist only under their unit flags (HIP_UNITS in build.py), for instance
vg_batch_i8.hip -DVGI_TU_PRE, vg_batch_h.hip -DVGH_TU=1..8, vg_batch_hl.hip -DVGHL_TU=0..5.
--digest: one line per kernel - VGPRs, SGPRs, spilled VGPRs / SGPRs, scratch, static LDS and a hash of the kernel's instruction text
(comments stripped, local label numbers and mangled symbol names blanked), then the demangled name: two revisions of a unit whose
lines agree generate the same code."""
import hashlib
import re
import subprocess
import sys
import tempfile

src = sys.argv[1]
show_all = "--all" in sys.argv
digest = "--digest" in sys.argv
with tempfile.NamedTemporaryFile(suffix=".s") as f:
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value",
                           "-Wno-unused-result", "--cuda-device-only", "-S", "-o", f.name, src] +
                          [a for a in sys.argv[2:] if a.startswith("-D")], stderr=subprocess.DEVNULL)
    text = open(f.name).read()


def body_hash(name):
    body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(0)
    body = re.sub(r"\s*;.*", "", body)                     # comments
    body = re.sub(r"\.L(BB|func_end)\d+", r".L\1", body)   # the function's number in its local labels
    body = re.sub(r"_Z\w+", "SYM", body)                   # mangled names
    return hashlib.sha256(body.encode()).hexdigest()[:16]


meta = text[text.index("amdhsa.kernels:"):]
for blk in meta.split("  - .agpr_count:")[1:]:
    g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)
    name, vg, sp, scr = g("name"), int(g("vgpr_count")), int(g("vgpr_spill_count")), int(g("private_segment_fixed_size"))
    if show_all or digest or sp or scr:
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(ScanArgs)", "")
        if digest:
            print("%4d vgpr %4d sgpr %4d vspill %4d sspill %5d scratch %6d lds  %s  %s" % (
                vg, int(g("sgpr_count")), sp, int(g("sgpr_spill_count")), scr, int(g("group_segment_fixed_size")), body_hash(name), dem))
        else:
            print("%4d vgpr %4d spilled %5d scratch  %s" % (vg, sp, scr, dem))
