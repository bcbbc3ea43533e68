"""fix spring/self and fix addforce on a decomposed run: two z slabs, one process per rank, against the same script on one GPU -
the comparison and the bounds of test_walls_across_slabs (test_gpu_wall_steps.py).  The input is the start of the recorded
crossing (extforce_runs.py); the members are the six beads that reach each of the two slab faces soonest - the plane between the slabs and
the periodic face, which is a slab face too - and are pulled across them, so that tethered beads change their owner, and some
of them their image flag, inside the run.  The LE lines are those of the recorded slab scenarios (reference_runs._DD: a ghost cutoff of
3.3, which two slabs of this box admit, and extruder bonds that stay inside it)."""
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import extforce_runs as ex
import reference_runs as rr
from dd_extforce_worker import STATS as DD_STATS
from dd_extforce_worker import results
from systems import run_product
from test_gpu_extforce import set_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PULL = 5.0


NEAR = 6


def soonest_at(system, plane):
    """The NEAR beads that reach the plane z = `plane` from below soonest at their starting velocity (no chain end)."""
    z, vz = np.asarray(system["x"])[:, 2], np.asarray(system["v"])[:, 2]
    t = np.where((vz > 0.2) & (z < plane), (plane - z) / np.maximum(vz, 1e-300), np.inf)
    t[0] = t[-1] = np.inf
    return [int(i) + 1 for i in np.argsort(t)[:NEAR]]


def dd_case():
    fx = ex.fixture("crossing")
    system = fx.system()
    box = np.asarray(system["box"])
    mid, top = 0.5 * (box[2, 0] + box[2, 1]), box[2, 1]
    a, b = soonest_at(system, mid), soonest_at(system, top)
    assert not set(a) & set(b)
    script = rr._DD + ("group edge id %s\nfix s edge spring/self 2.0\nfix_modify s energy yes\nfix a edge addforce 0.0 0.0 %.17g\n"
                       "fix_modify a energy yes virial yes\n" % (" ".join(str(i) for i in a + b), PULL))
    script += "thermo_style custom " + " ".join(("step",) + rr.THERMO) + "\nrun %d\n" % ex.B_STEPS
    return script, system, np.array(a) - 1, np.array(b) - 1, mid


def test_extforce_across_slabs(tmp_path, monkeypatch):
    """Bond tables, types, image flags, the LE fixes' counters, list builds, FENE warnings and the steps' paths identical; x to
    1e-9, v to 1e-8, every thermo column, pe and the fixes' sums (relative to max(1, |value|)) to 1e-9."""
    set_env(monkeypatch, {})
    script, system, a, b, mid = dd_case()
    p = run_product(script, system, tmp_path)
    one = results(p)
    p.close()
    session = uuid.uuid4().hex[:12]
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out.npz"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dd_extforce_worker.py"), str(r), "2", session, sysfile, scriptfile, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    assert all(q.returncode == 0 for q in procs), "\n".join(logs)
    r = np.load(out)
    st, st1 = dict(zip(DD_STATS, r["stats"])), dict(zip(DD_STATS, one["stats"]))
    assert st["comm_nranks"] == 2 and 0 < st["nlocal"] < len(system["x"])
    for k in DD_STATS[:7]:
        assert st[k] == st1[k], (k, st[k], st1[k])
    assert st["steps_fused_ext"] == 43 and st["steps_unfused"] == 5
    for q in ("num_bond", "bond_type", "bond_atom", "type", "image", "f_loop", "f_loading", "f_unloading"):
        assert np.array_equal(r[q], one[q]), q
    # the members did what they are here for: one went from the lower slab to the upper, one through the periodic face
    # (six members start below each face and head for it; which of them get through is the run's business)
    assert (system["x"][a, 2] < mid).all() and (r["x"][a, 2] >= mid).any()
    assert (r["image"][b, 2] == system["image"][b, 2] + 1).any()
    print("2 slabs: x %.2e v %.2e rows %.2e fixes %.2e" % (np.abs(r["x"] - one["x"]).max(), np.abs(r["v"] - one["v"]).max(),
                                                           np.abs(r["rows"] - one["rows"]).max(), np.abs(r["ext"] - one["ext"]).max()))
    assert np.abs(r["x"] - one["x"]).max() < 1e-9
    assert np.abs(r["v"] - one["v"]).max() < 1e-8
    assert r["rows"].shape == one["rows"].shape and np.abs(r["rows"] - one["rows"]).max() < 1e-9
    assert abs(r["pe"][0] - one["pe"][0]) < 1e-9
    assert (np.abs(r["ext"] - one["ext"]) / np.maximum(1.0, np.abs(one["ext"]))).max() < 1e-9 and np.abs(one["ext"]).max() > 0
