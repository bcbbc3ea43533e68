"""Nothing outlives a handle: every device block, pinned block, stream and event of an engine instance belongs to its
registry (DevMem, csrc/device.h) and is gone after close().  The test hook lammps_le_test_live_resources counts, over the
whole process, the live blocks, their bytes and the live streams + events; each test takes the three numbers before it opens
a handle and asserts the same three after close() plus gc.collect()."""
import ctypes
import gc

import numpy as np
import pytest

from systems import CHAIN_SCRIPT, lattice_chain, run_product
from test_gpu_angle import ANGLE_SCRIPT, semiflexible
from test_gpu_dd import run_ranks_local

pytestmark = pytest.mark.gpu


def live():
    from lammps_le_amd import library_path
    gc.collect()                     # handles that earlier tests dropped without close() go now, not in the middle of this test
    out = (ctypes.c_longlong * 3)()
    ctypes.CDLL(library_path()).lammps_le_test_live_resources(out)
    return tuple(out)


FEATURES = """angle_style harmonic
angle_coeff 1 3.0 170.0
angle_coeff 2 1.0 100.0
group hot id 1:3000:2
fix 1 all nve
fix 2 hot langevin 1.0 1.0 1.0 904297
fix loop all extrusion 7 1 1 1 1.0 2
fix loading all ex_load 5 1 1 1.12 2 prob 0.3 684474 iparam 1 1 jparam 1 1 atype 2
fix unloading all ex_unload 6 2 0.5 prob 0.4 456456
thermo 10
"""


def test_one_gpu_handle_leaves_nothing(tmp_path, monkeypatch):
    """One handle through: fix langevin on a group in batch and in block mode, `atom_modify sort`, an angle style, the three LE
    fixes, a subset gather and scatter, a neighbor-table regrowth, run_style respa, and a `neighbor` skin that changes the
    cell grid between two runs (the upload that follows allocates everything anew).  device_bytes: positive during a run,
    the same after a second identical run, and after the re-allocating change exactly what a fresh handle holds that had
    the new skin from the start (dev_free lets every block go, grow-only ones included, so no allowance is needed)."""
    monkeypatch.delenv("LAMMPS_LE_RNG_MODE", raising=False)
    monkeypatch.delenv("LAMMPS_LE_TEST_OVERFLOW_AT", raising=False)
    before = live()
    s = semiflexible(3000, 3, seed=9)
    script = ANGLE_SCRIPT.replace("atom_modify sort 0 0", "atom_modify sort 5 0") + FEATURES
    p = run_product(script + "run 20\n", s, tmp_path)
    b1 = p.stat("device_bytes")
    assert b1 > 0 and live()[1] - before[1] >= b1
    p.command("run 20")
    assert p.stat("device_bytes") == b1
    ids = np.arange(1, 3001, 7, dtype=np.int32)
    x = p.gather_ids("x", ids)
    p.scatter_ids("x", ids, x)
    assert p.stat("device_bytes") > b1                       # the staging block of the subset calls
    monkeypatch.setenv("LAMMPS_LE_TEST_OVERFLOW_AT", "0")    # the table is shrunk before build 0 of the run and grown again
    p.command("run 10")
    monkeypatch.delenv("LAMMPS_LE_TEST_OVERFLOW_AT")
    b_old = p.stat("device_bytes")
    monkeypatch.setenv("LAMMPS_LE_RNG_MODE", "block")        # read when fix langevin sets its generator up again: after the
    p.command("neighbor 0.8 bin")                            # re-allocation that the new cell grid brings with the next upload
    p.scatter("v", p.gather("v"))                            # (a whole-system scatter: the next run uploads)
    p.command("run 20")
    b_re = p.stat("device_bytes")
    assert b_re < b_old                                      # anew: the batch generator's pools are gone, and the grown table
    fresh = run_product(script.replace("neighbor 0.4 bin", "neighbor 0.8 bin") + "run 20\n", s, tmp_path)
    assert fresh.stat("device_bytes") == b_re
    fresh.close()
    p.command("run_style respa 2 3")
    p.command("run 12")
    assert p.stat("device_bytes") > b_re                     # the levels' force arrays
    assert live()[2] > before[2]
    p.close()
    assert live() == before


@pytest.mark.parametrize("world", [2, 3])
def test_in_process_ranks_leave_nothing(tmp_path, world):
    """Two and three slabs as threads of this process, Langevin and `atom_modify sort`: the segment tables of the batch
    generator (rng_need ..), the spare send lists and comm_stream with its events exist, and go with the handles."""
    before = live()
    s = lattice_chain(20000, nchains=2, seed=21)
    script = CHAIN_SCRIPT.replace("comm_modify cutoff 5.0", "comm_modify cutoff 2.0").replace("atom_modify sort 0 0", "atom_modify sort 10 0") + \
        "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nthermo 30\nrun 40\n"
    r = run_ranks_local(world, s, script, tmp_path)
    assert np.isfinite(r["x"]).all()
    assert live() == before


def test_failed_run_leaves_nothing(tmp_path):
    """A run that ends in a host-side error (Bad FENE bond, as in test_gpu_misc.py), then close()."""
    from lammps_le_amd import LammpsError
    before = live()
    s = lattice_chain(2000, seed=35)
    s["x"][1000] += np.array([3.2, 0.0, 0.0])          # stretch two backbone bonds far beyond 2*R0
    p = run_product(CHAIN_SCRIPT + "fix 1 all nve\n", s, tmp_path)
    with pytest.raises(LammpsError, match="Bad FENE bond"):
        p.command("run 5")
    assert p.stat("device_bytes") > 0
    p.close()
    assert live() == before
