"""Who may allocate and free device memory in csrc/ (driver.hpp): the owner DevArr, the communicator, and the
few C entries that hand a raw device pointer to their caller.  Read from the sources, so no GPU is needed."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyamg_amd", "csrc")

# whole files: the owner itself, and the communicator (arena, tickets and send buffers live as long as peers and IPC handles do)
FILES = {"driver.hpp", "comm.hip"}
# C entries whose buffer belongs to the caller
MAY_ALLOCATE = {"amg_dev_alloc", "amg_hierx_vec_alloc"}
MAY_FREE = {"amg_dev_free", "amg_hierx_vec_alloc", "amg_hierx_vec_free"}        # vec_alloc: its own failed fill


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))


def _enclosing_function(lines, k):
    """name of the function whose definition starts at column 0 at or above line k"""
    for q in range(k, -1, -1):
        m = re.match(r"^[A-Za-z_][^;]*?\b(\w+)\(", lines[q])
        if m:
            return m.group(1)
    return None


def _sites(text):
    out = []
    for path in _sources():
        name = os.path.basename(path)
        if name in FILES:
            continue
        with open(path) as f:
            lines = f.read().split("\n")
        for k, line in enumerate(lines):
            if text in line:
                out.append((name, k + 1, _enclosing_function(lines, k)))
    return out


def test_library_loads_and_holds_nothing():
    from pyamg_amd import _lib
    assert _lib.live_buffers() == 0


def test_sources_are_there():
    assert len(glob.glob(os.path.join(CSRC, "*.hip"))) == 21 and os.path.exists(os.path.join(CSRC, "driver.hpp"))


def test_frees_only_in_the_owner_and_at_the_boundary():
    stray = [s for s in _sites("hipFree(") if s[2] not in MAY_FREE]
    assert not stray, stray
    assert {s[2] for s in _sites("hipFree(")} == MAY_FREE


def test_allocations_only_in_the_owner_and_at_the_boundary():
    stray = [s for s in _sites("hipMalloc(") if s[2] not in MAY_ALLOCATE]
    assert not stray, stray
    assert {s[2] for s in _sites("hipMalloc(")} == MAY_ALLOCATE


@pytest.mark.parametrize("name", ["amg_dev.hpp", "hier.hpp", "spgemm.hip"])
def test_no_ownership_flags(name):
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    assert not re.search(r"\b\w*owned\b\s*(=[^=]|;)", text)
    assert "Ablk_owned" not in text
