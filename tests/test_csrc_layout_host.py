"""
The layout of mininf_amd/csrc: every unit is built, the site planner's unit holds no kernel of the
units split out of it, and no file grows back to the size of the undivided sites.hip.
"""
import glob
import os
import re

from mininf_amd import build

# sites.hip before it was split into sites / bcast_site / reduce / categorical
UNDIVIDED_SITES_LINES = 2267


def test_every_unit_is_built():
    for path in build.SOURCES:
        assert os.path.isfile(path), path
    listed = {os.path.realpath(path) for path in build.SOURCES}
    for path in glob.glob(os.path.join(build.CSRC, "*.hip")):
        assert os.path.realpath(path) in listed, path


def test_sites_unit_holds_only_the_group_kernels():
    text = open(os.path.join(build.CSRC, "sites.hip")).read()
    # a kernel definition: __global__, launch bounds or none, `void name(`
    defined = set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", text))
    assert defined, "no kernel definition found: the search is broken"
    for name in ("k_site_bcast", "k_finalize", "k_categorical"):
        assert not any(kernel.startswith(name) for kernel in defined), (name, sorted(defined))


def test_no_file_is_as_long_as_the_undivided_sites_unit():
    paths = glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.hpp"))
    assert paths
    for path in paths:
        with open(path) as fh:
            lines = sum(1 for _ in fh)
        assert lines <= UNDIVIDED_SITES_LINES, (path, lines)
