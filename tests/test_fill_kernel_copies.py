"""k_raster_fill's register copies, read from the compiler's assembly (no GPU): a guard against the copies of the sixteen colour registers and the
four winding cells coming back with the next edit of the walk. The kernel is bound by vector-instruction issue, and a copy is an
instruction: the parent of this test's commit ran 36 of them per cover entry around a blend of 16 to 32.

raster_edges.hip is compiled device-only to assembly with build.py's flags. For k_raster_fill<true, 7, false> and <true, 7, true>:
  * 72 vector registers at the most and no scratch memory (the seven-wave build);
  * no basic block of eight or more VGPR-to-VGPR v_mov_b32 and nothing else;
  * the VGPR-to-VGPR v_mov_b32 outside inline asm (the opaque blend's own sixteen are the statement's work) within the budget below.
The test looks for nothing but v_mov_b32."""
import os
import re
import shutil
import subprocess

import pytest

from contrast_renderer_amd.build import CSRC, FILE_FLAGS, FLAGS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc")

pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not installed")

# The counts the finished kernels reach with the toolchain this was written with (ROCm 7.0.2): VGPR-to-VGPR v_mov_b32 outside inline asm, whole kernel.
# The parent had 103 and 105; the single blend statement alone gives 55 and 57, the curve kinds as four lone ifs the rest. What is left: four at the
# group loop's back edge behind a cover (the cover's three arms), the others in the sorts and the chunk set-up in front of the walk.
COPY_BUDGET = {"_ZN3crh13k_raster_fillILb1ELi7ELb0EEEvNS_8SceneDevENS_12RasterParamsE": 19, "_ZN3crh13k_raster_fillILb1ELi7ELb1EEEvNS_8SceneDevENS_12RasterParamsE": 21}
COPY = re.compile(r"^v_mov_b32(?:_e32)?\s+v\d+,\s*v\d+\s*$")
ENDS_BLOCK = re.compile(r"^(s_cbranch_|s_branch|s_endpgm|s_setpc|s_swappc)")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    out = tmp_path_factory.mktemp("fill_asm") / "raster_edges.s"
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get("raster_edges.hip", []) + ["-Wno-pass-failed", "--cuda-device-only", "-S", os.path.join(CSRC, "raster_edges.hip"), "-o", str(out)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    return out.read_text()


def kernel_text(assembly, symbol):
    """(the kernel's instructions, {num_vgpr, private_seg_size, ...} of the `.set symbol.name, value` lines behind them)"""
    start = assembly.index("\n" + symbol + ":")
    body = assembly[start:assembly.index(".Lfunc_end", start)]
    figures = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set\s+" + re.escape(symbol) + r"\.(\w+),\s*(\d+)\s*$", assembly, re.M)}
    return body, figures


def blocks_of(body):
    """Basic blocks as lists of (instruction, inside inline asm): cut at labels and behind branches."""
    blocks, cur, in_asm = [], [], False
    for raw in body.splitlines():
        line = raw.strip()
        if line.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if line.startswith(";;#ASMEND"):
            in_asm = False
            continue
        line = line.split(";")[0].strip()
        if not line or line.startswith("."):
            if re.match(r"^\.L\w+:", line) and cur:
                blocks.append(cur)
                cur = []
            continue
        if re.match(r"^[\w.$]+:$", line):
            if cur:
                blocks.append(cur)
                cur = []
            continue
        if ENDS_BLOCK.match(line):
            blocks.append(cur)
            cur = []
            continue
        cur.append((line, in_asm))
    if cur:
        blocks.append(cur)
    return [b for b in blocks if b]


@pytest.mark.parametrize("symbol", sorted(COPY_BUDGET))
def test_fill_kernel_registers_and_copies(assembly, symbol):
    body, figures = kernel_text(assembly, symbol)
    vgprs, scratch = figures["num_vgpr"], figures["private_seg_size"]
    blocks = blocks_of(body)
    copies = sum(1 for b in blocks for line, in_asm in b if not in_asm and COPY.match(line))
    copy_blocks = [len(b) for b in blocks if len(b) >= 8 and all(COPY.match(line) for line, _ in b)]
    print(f"{symbol}: vgpr {vgprs} scratch {scratch} copies outside asm {copies} copy-only blocks {copy_blocks}")
    assert vgprs <= 72
    assert scratch == 0
    assert copy_blocks == [], "a block of nothing but register copies: the colour registers are being moved around the blend again"
    assert copies <= COPY_BUDGET[symbol]
