"""Builds libcontrast_hip.so in-tree with hipcc for gfx950 (the .so travels to the GPU box with the snapshot).

-ffp-contract=off is part of the numerical contract: Rust never fuses a*b+c, and the parity tests compare bytes.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ("tessellate.hip", "raster.hip", "bin_edges.hip", "raster_edges.hip", "image_filter.hip", "api.hip", "image.hip", "comm.hip", "text.cpp", "path.cpp")  # text.cpp / path.cpp: host-only (text.rs, path.rs:639-708)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-bitwise-instead-of-logical"]
# Per-file flags. raster_edges.hip and bin_edges.hip (one file when this was measured) without LLVM's SLP vectorizer (round 6): it packs pairs of independent f32 operations of the per-sample code into
# v_pk_* instructions, whose operands are register PAIRS — lane-invariant values (sample positions, the tile's origin) end up duplicated in pairs that live
# for the whole kernel, and the raster kernels spilled exactly those (k_raster_edges<4,1,true,false>: 100 B of scratch per lane -> 12, 96 -> 95 registers;
# k_raster_fill 94 -> 76 registers; k_raster_rows 112 -> 95). Same results bit for bit (no contraction either way); S10k raster kernel 0.166 -> 0.151 ms alone,
# dashed scene 1.557 -> 1.481 (profiles/r06_experiments.txt). CRH_FILE_FLAGS="file.hip:-flag,-flag;..." replaces the table (A/B runs).
FILE_FLAGS = {"raster_edges.hip": ["-fno-slp-vectorize"], "bin_edges.hip": ["-fno-slp-vectorize", "-mllvm", "-disable-machine-licm"], "raster.hip": ["-fno-slp-vectorize", "-mllvm", "-pragma-unroll-threshold=65536"], "tessellate.hip": ["-fno-slp-vectorize"]}  # (raster.hip: k_raster_tile<4,1,true,true> 150 -> 127 registers; tessellate.hip: k_tess_runs<true> 182 -> 146)
# bin_edges.hip without LLVM's machine-level loop-invariant code motion: k_bin_flat's body is a loop over the workgroup's batches that nearly always runs once,
# and the pass moved some forty constants and table offsets in front of it, into vector registers that then lived through all eight phases — at 128 registers
# (four waves per SIMD) the kernel spilled 28 B per lane for them; without the pass it needs 125 and no scratch memory.
# raster.hip also raises LLVM's size limit for `#pragma unroll` (16384 by default): the body's turn loop in k_raster_mip<8, ...> is larger, and a loop that
# stays rolled indexes the per-sample arrays at run time, which puts them in scratch (144 B per lane). The kernels that unrolled before are unchanged by it.
OUT = os.path.join(HERE, "libcontrast_hip.so")


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps if os.path.exists(d))


def header_deps():
    """What every object is rebuilt after: each header csrc/ holds and the two public ones the sources include. Listed from the directory, so that a
    new header cannot be forgotten (a missing one made _newer reuse a stale object silently)."""
    own = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h", ".inc")))
    return own + [os.path.join(HERE, "..", "include", h) for h in ("contrast_hip.h", "crh_fmath.h")]


def file_flags():
    table = os.environ.get("CRH_FILE_FLAGS")
    if table is None:
        return FILE_FLAGS
    out = {}
    for entry in filter(None, table.split(";")):
        name, _, flags = entry.partition(":")
        out[name] = [f for f in flags.split(",") if f]
    return out


def build_library(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    headers = header_deps()
    objects = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(HERE, "build", os.path.splitext(src)[0] + ".o")
        objects.append(obj)
        if not force and _newer(obj, [os.path.join(CSRC, src)] + headers):
            continue
        flags = (FLAGS + os.environ.get("CRH_EXTRA_FLAGS", "").split()) if src.endswith(".hip") else [f for f in FLAGS if not f.startswith("--offload-arch")]  # plain C++ for host-only files
        flags = flags + file_flags().get(src, [])
        cmd = [hipcc] + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, proc in procs:
        out, _ = proc.communicate()
        if proc.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
        if verbose and out:
            print(out.decode(), file=sys.stderr)
    exports = write_export_map()
    if procs or not os.path.exists(OUT) or os.path.getmtime(exports) > os.path.getmtime(OUT):
        # librccl.so is dlopen()ed by comm.hip, not linked; the version script keeps the dynamic symbol table to the C ABI
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objects + ["-ldl", "-Wl,--version-script=" + exports, "-o", OUT]
        subprocess.check_call(cmd)
    return OUT


DEBUG_TAPS = ("crh_debug_frame_counters", "crh_debug_frame_counters16", "crh_debug_frame_words", "crh_debug_frame_bin_dump", "crh_debug_flat_batches", "crh_debug_pass_leaves_state",
              "crh_debug_frame_last_pass", "crh_debug_frame_tile_place")  # tools/ and the tests read the raster kernels' counters through these


def declared_entry_points():
    """The names include/contrast_hip.h declares — the whole of the library's dynamic symbol table, with the debug taps."""
    import re
    with open(os.path.join(HERE, "..", "include", "contrast_hip.h")) as f:
        return sorted(set(re.findall(r"\b(crh_[a-z_0-9]+)\s*\(", f.read())) - {"crh_status"})


def write_export_map():
    """build/exports.map: a linker version script listing exactly the header's entry points. Everything else — the C++ internals shared by
    the translation units (crh::launch_*), the crh_internal_* accessors comm.hip uses, HIP's kernel stubs — stays local to the library."""
    path = os.path.join(HERE, "build", "exports.map")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    text = "{\n  global:\n" + "".join(f"    {name};\n" for name in declared_entry_points() + list(DEBUG_TAPS)) + "  local:\n    *;\n};\n"
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
