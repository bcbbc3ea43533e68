"""The one walk over the fixes that places every post-force fix of a run (PostForce::build, csrc/post_force.cpp), without a
device: test hook lammps_le_test_post_force_rows - the init() of a run command, then the walk; per post-force fix, in fix order,
family (0 wall/region, 1 indent, 2 spring/self | addforce | setforce), index within its table, phase, group bit.

One fix each of wall/region, indent, spring/self, addforce, setforce and langevin behind a fix nve, in every one of the 720
orders.  What must come back follows from the order of the script alone: a fix is in phase 1 exactly when it is defined behind
fix langevin; the run is refused, in the words of the first wall or indenter that has an addforce or setforce ahead of it on its
side of fix langevin, exactly when there is one; otherwise the rows come back in fix order, each family counting its own."""
import ctypes
import itertools
import os
import re

import pytest

from systems import CHAIN_SCRIPT, lattice_chain, write_data

LINES = {"w": "fix w all wall/region inside lj126 1.0 1.0 1.12", "c": "fix c some indent 5.0 sphere 1.0 1.0 1.0 0.5 side out",
         "s": "fix s some spring/self 2.0", "a": "fix a all addforce 0.1 0.0 0.0 every 3", "z": "fix z few setforce 0.0 NULL 0.0",
         "l": "fix l all langevin 1.0 1.0 1.0 4242"}
FAMILY = {"w": 0, "c": 1, "s": 2, "a": 2, "z": 2}
GROUPBIT = {"w": 1, "c": 2, "s": 2, "a": 1, "z": 4}          # all, some (the first group defined), few (the second)
REFUSAL = {"w": "MI355X engine: fix w (wall/region) is defined behind a fix addforce or setforce on the same side of fix langevin; define the wall first",
           "c": "MI355X engine: fix c (indent) is defined behind a fix addforce or setforce on the same side of fix langevin; define the indenter first"}


def expected(order):
    """(rows, None) or (None, the refusal) of the fixes `order` (letters of LINES) from their order alone."""
    behind = lambda k: "l" in order[:k]
    for k, f in enumerate(order):
        if f in "wc" and any(g in "az" and behind(j) == behind(k) for j, g in enumerate(order[:k])):
            return None, REFUSAL[f]
    rows, count = [], [0, 0, 0]
    for k, f in enumerate(order):
        if f == "l":
            continue
        rows.append((FAMILY[f], count[FAMILY[f]], int(behind(k)), GROUPBIT[f]))
        count[FAMILY[f]] += 1
    return rows, None


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    from lammps_le_amd import lammps, library_path
    path = os.path.join(str(tmp_path_factory.mktemp("walk")), "data.chain")
    s = lattice_chain(125)
    write_data(path, s)
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in CHAIN_SCRIPT.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    lmp.command("group some id 1:125:2")
    lmp.command("group few id 3:5")
    lmp.command("region inside block INF INF INF INF INF INF")
    fn = ctypes.CDLL(library_path()).lammps_le_test_post_force_rows
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 64)()

    def rows(order):
        """The hook's answer for the fixes `order` behind a fix nve; every fix is deleted again."""
        for f in ["fix 1 all nve"] + [LINES[k] for k in order]:
            lmp.command(f)
        try:
            n = fn(lmp.lmp, out)
            lmp._check()
            return [tuple(out[4 * k:4 * k + 4]) for k in range(n)]
        finally:
            for f in ["1"] + list(order):
                lmp.command("unfix " + f)
    yield lmp, rows, lambda: (fn(lmp.lmp, out), lmp._check())[0]
    lmp.close()


def test_every_order(handle):
    from lammps_le_amd import LammpsError
    _, rows, _ = handle
    refused = 0
    for order in itertools.permutations("wcsazl"):
        want, refusal = expected(order)
        if refusal is None:
            assert rows(order) == want, order
        else:
            refused += 1
            with pytest.raises(LammpsError, match="^" + re.escape(refusal) + "$"):
                rows(order)
    assert 0 < refused < 720
    # the model itself, at three orders written out by hand
    assert expected("wcsalz") == ([(0, 0, 0, 1), (1, 0, 0, 2), (2, 0, 0, 2), (2, 1, 0, 1), (2, 2, 1, 4)], None)
    assert expected("alwcsz") == ([(2, 0, 0, 1), (0, 0, 1, 1), (1, 0, 1, 2), (2, 1, 1, 2), (2, 2, 1, 4)], None)
    assert expected("awlcsz") == (None, REFUSAL["w"]) and expected("alwzcs") == (None, REFUSAL["c"])


def test_without_langevin_and_after_unfix(handle):
    _, rows, bare = handle
    got = rows("wcsaz")
    assert got == [(0, 0, 0, 1), (1, 0, 0, 2), (2, 0, 0, 2), (2, 1, 0, 1), (2, 2, 0, 4)]
    assert bare() == 0          # (rows() has deleted every fix: the same handle reports none)
