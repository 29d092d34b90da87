"""In-tree native build for the MI355X scan path.

    libvectorgpu.so : hipcc --offload-arch=gfx950 over csrc/*.hip     (HIP kernels + C-ABI)
    vector.so       : gcc over ext/vector_ext.c                       (SQLite loadable extension, plain C)

hipcc cross-compiles without a GPU.  The extension needs no SQLite development headers: ext/vext_sqlite.h declares the
part of SQLite's public interface it uses, and it reaches SQLite through the routines table its host hands it.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
EXT = os.path.join(HERE, "ext")
LIB = os.path.join(HERE, "libvectorgpu.so")
VEC = os.path.join(HERE, "vector.so")

# (source, object, extra flags): the two kernel families with the most template instantiations are compiled as several
# translation units from one source file each (the half-precision batch kernels: 9 + 6 units), so that a from-scratch build is bounded
# by the total CPU time over the cores (~30 CPU-minutes: ~4 min on 8 cores) instead of by its longest unit
HIP_UNITS = [("vg_api.hip", "vg_api.hip.o", []), ("vg_corpus.hip", "vg_corpus.hip.o", []), ("vg_batch_api.hip", "vg_batch_api.hip.o", []),
             ("vg_select.hip", "vg_select.hip.o", []), ("vg_batch.hip", "vg_batch.hip.o", []), ("vg_quant.hip", "vg_quant.hip.o", []),
             ("vg_shards.hip", "vg_shards.hip.o", []), ("vg_multi.hip", "vg_multi.hip.o", []), ("vg_reforder.hip", "vg_reforder.hip.o", []), ("vg_slabscan.hip", "vg_slabscan.hip.o", []), ("vg_scan_ex.hip", "vg_scan_ex.hip.o", []), ("vg_scan_within.hip", "vg_scan_within.hip.o", []), ("vg_scan_masked.hip", "vg_scan_masked.hip.o", []), ("vg_multi_masked.hip", "vg_multi_masked.hip.o", []), ("vg_multi_within.hip", "vg_multi_within.hip.o", []), ("vg_scan_within_masked.hip", "vg_scan_within_masked.hip.o", []), ("vg_multi_within_masked.hip", "vg_multi_within_masked.hip.o", []), ("vg_multi_within_labeled.hip", "vg_multi_within_labeled.hip.o", []), ("vg_scan_after.hip", "vg_scan_after.hip.o", []), ("vg_multi_after.hip", "vg_multi_after.hip.o", []), ("vg_rowpred.hip", "vg_rowpred.hip.o", []), ("vg_multi_labeled.hip", "vg_multi_labeled.hip.o", []), ("vg_multi_labelset.hip", "vg_multi_labelset.hip.o", []), ("vg_multi_valued.hip", "vg_multi_valued.hip.o", []), ("vg_scan_grouped.hip", "vg_scan_grouped.hip.o", []), ("vg_multi_grouped.hip", "vg_multi_grouped.hip.o", []), ("vg_multi_grouped_masked.hip", "vg_multi_grouped_masked.hip.o", []), ("vg_scan_capped.hip", "vg_scan_capped.hip.o", []), ("vg_multi_capped.hip", "vg_multi_capped.hip.o", []), ("vg_multi_capped_masked.hip", "vg_multi_capped_masked.hip.o", []), ("vg_filter.hip", "vg_filter.hip.o", []),
             ("vg_batch_q8.hip", "vg_batch_q8.o", []),
             ("vg_batch_i8.hip", "vg_batch_i8.hip.o", []), ("vg_batch_i8.hip", "vg_batch_i8_pre.o", ["-DVGI_TU_PRE"]),
             ("vg_batch_h.hip", "vg_batch_h.hip.o", []), ("vg_batch_h.hip", "vg_batch_h_bf16.o", ["-DVGH_TU=1"]),
             ("vg_batch_h.hip", "vg_batch_h_bound.o", ["-DVGH_TU=2"]), ("vg_batch_h.hip", "vg_batch_h_f32.o", ["-DVGH_TU=3"]),
             ("vg_batch_h.hip", "vg_batch_h_bound_bf16.o", ["-DVGH_TU=4"]), ("vg_batch_h.hip", "vg_batch_h_bound_f32.o", ["-DVGH_TU=5"]),
             ("vg_batch_h.hip", "vg_batch_h_split_f16.o", ["-DVGH_TU=6"]), ("vg_batch_h.hip", "vg_batch_h_split_bf16.o", ["-DVGH_TU=7"]),
             ("vg_batch_h.hip", "vg_batch_h_split_f32.o", ["-DVGH_TU=8"])] + \
            [("vg_batch_hl.hip", "vg_batch_hl_%d.o" % tu, ["-DVGHL_TU=%d" % tu]) for tu in range(6)]
HIP_SOURCES = sorted(set(u[0] for u in HIP_UNITS))
# --offload-compress: the gfx950 code objects are stored zstd-compressed inside the host objects (round 6: libvectorgpu.so 26.8 -> ~8 MB; the
# runtime inflates a code object once, when the library is loaded)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result"] + \
              ([] if os.environ.get("VG_BUILD_NO_COMPRESS") else ["--offload-compress"])


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build the gfx950 kernels)")


def build_gpu_library(force=False, verbose=False):
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(ROOT, "include", "vectorgpu.h"), os.path.join(ROOT, "include", "vectorgpu_diag.h")]
    if not force and not _newer(LIB, srcs + hdrs):
        return LIB
    # one object per translation unit (compiled concurrently), then one link
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    objs, procs = [], []
    for name, objname, extra in HIP_UNITS:
        src = os.path.join(CSRC, name)
        obj = os.path.join(HERE, "build", objname)
        objs.append(obj)
        if force or _newer(obj, [src] + hdrs):           # an object depends on its own source + every header
            cmd = [_hipcc()] + HIPCC_FLAGS + extra + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=CSRC)
    return LIB


def build_extension(force=False, verbose=False):
    src = os.path.join(EXT, "vector_ext.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(ROOT, "include", "vectorgpu.h")] + [os.path.join(EXT, f) for f in os.listdir(EXT) if f.endswith((".inc", ".h"))]
    if not force and not _newer(VEC, deps):
        return VEC
    cmd = ["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-missing-field-initializers",
           "-I" + os.path.join(ROOT, "include"), "-I" + EXT, "-o", VEC, src, "-ldl", "-lm", "-lpthread"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return VEC


def build_all(force=False, verbose=False):
    build_gpu_library(force, verbose)
    build_extension(force, verbose)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
