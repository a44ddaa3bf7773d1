"""Configuration::blending (renderer.rs:380-382) without a GPU: the C ABI refuses what WebGPU's pipeline validation refuses before any device
is touched, and the Python and C++ mirrors build the same crh_color_target_state field for field."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

from contrast_renderer_amd import _ffi
from contrast_renderer_amd.renderer import (BlendComponent, BlendFactor, BlendOperation, BlendState, ColorTargetState, ColorWrites, Configuration)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVER = BlendComponent.OVER
ADD = BlendComponent(BlendFactor.One, BlendFactor.One, BlendOperation.Add)


def create(state, lib):
    cfg = _ffi.ConfigC(1, 4, 4, 0)
    handle = C.c_void_p()
    rc = lib.crh_renderer_create_blended(C.byref(cfg), C.byref(state), 0, C.byref(handle))
    if rc == _ffi.OK:  # (a machine with a GPU)
        lib.crh_renderer_destroy(handle)
    return rc


def state_with(**fields):
    s = ColorTargetState(BlendState.PREMULTIPLIED_ALPHA_BLENDING).to_c()
    for name, value in fields.items():
        part, _, field = name.partition("_")
        if part in ("color", "alpha"):
            setattr(getattr(s, part), field, value)
        elif name == "constant0":
            s.constant[0] = value
        else:
            setattr(s, name, value)
    return s


REFUSED = [
    ("color src factor 17", dict(color_src_factor=17), _ffi.ERR_INVALID_ARGUMENT),
    ("alpha dst factor 17", dict(alpha_dst_factor=17), _ffi.ERR_INVALID_ARGUMENT),
    ("color operation 5", dict(color_operation=5), _ffi.ERR_INVALID_ARGUMENT),
    ("alpha operation 5", dict(alpha_operation=5), _ffi.ERR_INVALID_ARGUMENT),
    ("write mask 16", dict(write_mask=16), _ffi.ERR_INVALID_ARGUMENT),
    ("constant nan", dict(constant0=math.nan), _ffi.ERR_INVALID_ARGUMENT),
    ("constant inf", dict(constant0=math.inf), _ffi.ERR_INVALID_ARGUMENT),
    ("min with over factors", dict(color_operation=BlendOperation.Min), _ffi.ERR_INVALID_ARGUMENT),
    ("max with over factors", dict(alpha_operation=BlendOperation.Max), _ffi.ERR_INVALID_ARGUMENT),
    ("min with a src factor", dict(color_operation=BlendOperation.Min, color_dst_factor=BlendFactor.One, color_src_factor=BlendFactor.SrcAlpha), _ffi.ERR_INVALID_ARGUMENT),
    ("dual source Src1", dict(color_src_factor=BlendFactor.Src1), _ffi.ERR_UNSUPPORTED),
    ("dual source OneMinusSrc1Alpha", dict(alpha_dst_factor=BlendFactor.OneMinusSrc1Alpha), _ffi.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("fields,status", [(f, s) for _, f, s in REFUSED], ids=[n for n, _, _ in REFUSED])
def test_the_c_abi_refuses_invalid_blend_states_before_touching_a_device(fields, status):
    assert create(state_with(**fields), _ffi.load_library()) == status


def test_valid_states_pass_validation():
    """A valid state gets past the checks: it fails only where a device is needed (no GPU) or succeeds (GPU)."""
    lib = _ffi.load_library()
    ok = (_ffi.OK, _ffi.ERR_HIP)  # (HipError: no device on this machine)
    for s in (state_with(color_operation=BlendOperation.Max, color_src_factor=BlendFactor.One, color_dst_factor=BlendFactor.One),
              state_with(blend_enabled=0, write_mask=0), state_with(constant0=-3.0), state_with(color_src_factor=BlendFactor.OneMinusConstant)):
        rc = create(s, lib)
        assert rc in ok, rc
    # the stencil-bit check comes first, as for crh_renderer_create
    cfg = _ffi.ConfigC(1, 5, 4, 0)
    assert lib.crh_renderer_create_blended(C.byref(cfg), C.byref(state_with(write_mask=16)), 0, C.byref(C.c_void_p())) == _ffi.ERR_NUMBER_OF_STENCIL_BITS_IS_UNSUPPORTED


def fields(c):
    return [c.blend_enabled, c.color.src_factor, c.color.dst_factor, c.color.operation, c.alpha.src_factor, c.alpha.dst_factor, c.alpha.operation,
            c.write_mask] + [float(v) for v in c.constant]


STATES = {
    "premultiplied": ColorTargetState(BlendState.PREMULTIPLIED_ALPHA_BLENDING),
    "alpha": ColorTargetState(BlendState.ALPHA_BLENDING, ColorWrites.RED | ColorWrites.ALPHA, (0.25, 0.5, 0.75, 1.0)),
    "replace": ColorTargetState(),
    "mixed": ColorTargetState(BlendState(ADD, BlendComponent(BlendFactor.Constant, BlendFactor.OneMinusConstant, BlendOperation.ReverseSubtract)),
                              ColorWrites.COLOR, (0.125, 0.0, 1.0, 0.5)),
}


def test_python_mirror_converts_field_for_field():
    assert fields(STATES["premultiplied"].to_c()) == [1, 1, 5, 0, 1, 5, 0, 15, 0.0, 0.0, 0.0, 0.0]
    assert fields(STATES["alpha"].to_c()) == [1, 4, 5, 0, 1, 5, 0, 9, 0.25, 0.5, 0.75, 1.0]
    assert fields(STATES["replace"].to_c())[0] == 0 and fields(STATES["replace"].to_c())[7] == 15
    assert fields(STATES["mixed"].to_c()) == [1, 1, 1, 0, 11, 12, 2, 7, 0.125, 0.0, 1.0, 0.5]
    for s in STATES.values():
        assert ColorTargetState.from_c(s.to_c()) == s
    assert C.sizeof(_ffi.ColorTargetStateC) == 4 * 12
    assert list(Configuration.__dataclass_fields__)[-1] == "blending" and Configuration().blending is None
    assert BlendState.REPLACE == BlendState() and BlendComponent() == BlendComponent.REPLACE
    assert [int(f) for f in BlendFactor] == list(range(17)) and [int(o) for o in BlendOperation] == list(range(5))


def test_cpp_mirror_with_blending_compiles_links_and_agrees_with_python():
    import __graft_entry__ as entry
    entry.build()
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "blend_harness")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "blend_harness.cpp"),
               "-o", exe, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr
        run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
    lines = {line.split()[0]: line.split()[1:] for line in run.stdout.splitlines()}
    for name, state in STATES.items():
        assert [float(v) for v in lines[name]] == [float(v) for v in fields(state.to_c())], name
    assert lines["plain"] == ["0"]
    assert lines["refused"] == [str(_ffi.ERR_INVALID_ARGUMENT), str(_ffi.ERR_UNSUPPORTED), str(_ffi.ERR_INVALID_ARGUMENT)]


def test_python_upload_refuses_a_wrong_size_before_the_library():
    from contrast_renderer_amd import ContrastError
    from contrast_renderer_amd.renderer import Frame
    import numpy as np
    f = Frame.__new__(Frame)
    f.width, f.height = 8, 4
    with pytest.raises(ContrastError) as e:
        Frame.upload(f, np.zeros((8, 4, 4), dtype=np.uint8))
    assert e.value.status == _ffi.ERR_INVALID_ARGUMENT
