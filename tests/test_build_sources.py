"""The build's bookkeeping (contrast_renderer_amd/build.py; no device, no compiler): every source of csrc/ is compiled, every header of csrc/
is a dependency of every object, the files whose kernels are built without the SLP vectorizer keep that flag, and the library exports exactly
the C ABI of include/contrast_hip.h with the debug taps."""
import os
import re

from contrast_renderer_amd import build


def test_sources_headers_file_flags_and_exports_are_complete():
    names = os.listdir(build.CSRC)
    sources = {f for f in names if f.endswith((".hip", ".cpp"))}
    assert sources == set(build.SOURCES) and len(set(build.SOURCES)) == len(build.SOURCES)

    deps = {os.path.realpath(d) for d in build.header_deps()}
    headers = {os.path.realpath(os.path.join(build.CSRC, f)) for f in names if f.endswith((".hpp", ".h", ".inc"))}
    public = {os.path.realpath(os.path.join(build.HERE, "..", "include", h)) for h in ("contrast_hip.h", "crh_fmath.h")}
    assert headers and headers <= deps and public <= deps
    assert all(os.path.isfile(d) for d in deps)

    for name in ("raster.hip", "tessellate.hip", "raster_edges.hip", "bin_edges.hip"):
        with open(os.path.join(build.CSRC, name)) as f:
            assert "__global__" in f.read(), name
        assert "-fno-slp-vectorize" in build.FILE_FLAGS.get(name, []), name

    with open(build.write_export_map()) as f:
        text = f.read()
    exported = re.findall(r"^\s+(crh_\w+);$", text.split("local:")[0], flags=re.M)
    assert exported == build.declared_entry_points() + list(build.DEBUG_TAPS)
    assert len(exported) == len(set(exported)) and text.split("local:")[1].split() == ["*;", "};"]
