"""fix indent on a decomposed run: two z slabs, one process per rank, against the same script on one GPU - the comparison and
the bounds of test_gpu_extforce_dd.py, on its input (the start of the recorded crossing of extforce_runs.py under the LE lines of
the recorded slab scenarios, reference_runs._DD).  A sphere-in indenter has its centre on the plane between the slabs and is
written one box length above it, so that Domain::remap acts; its radius leaves the corners of the box outside, on both slabs and
through every periodic face.  Each rank evaluates the beads it owns; the four sums join the all-reduce of the thermo row."""
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import extforce_runs as ex
import indent_reference as ir
import reference_runs as rr
from dd_indent_worker import STATS as DD_STATS
from dd_indent_worker import results
from systems import run_product
from test_gpu_indent import set_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K, RADIUS_OF_L = 5.0, 0.70


def dd_case():
    system = ex.fixture("crossing").system()
    box = np.asarray(system["box"], dtype=np.float64)
    L = box[:, 1] - box[:, 0]
    c = 0.5 * (box[:, 0] + box[:, 1])
    o = dict(kind="sphere", K=K, side="in", ctr=[c[0], c[1], c[2] + L[2]], R=float(np.round(RADIUS_OF_L * L[0], 3)))
    script = rr._DD + ("fix c all indent %.17g sphere %.17g %.17g %.17g %.17g side in units box\nfix_modify c energy yes\n"
                       % (K, o["ctr"][0], o["ctr"][1], o["ctr"][2], o["R"]))
    script += "thermo_style custom " + " ".join(("step",) + rr.THERMO) + "\nrun %d\n" % ex.B_STEPS
    return script, system, o, c[2]


def test_indent_across_slabs(tmp_path, monkeypatch):
    """Bond tables, types, image flags, the LE fixes' counters, list builds, FENE warnings and the steps' paths identical; x to
    1e-9, v to 1e-8, every thermo column, pe and the indenter's sums (relative to max(1, |value|)) to 1e-9.
    Measured on an MI355X: x 5.3e-15, v 1.8e-13, thermo rows 3.6e-15, the indenter's sums 7.1e-15 absolute."""
    set_env(monkeypatch, {})
    script, system, o, mid = dd_case()
    # the indenter touches beads of both slabs at the start, none of them by more than 1.5
    t = ir.terms(system["x"], o, system["box"])
    below = np.asarray(system["x"])[:, 2] < mid
    assert (t["touched"] & below).sum() >= 8 and (t["touched"] & ~below).sum() >= 8 and float(np.nanmin(t["dr"])) > -1.5
    assert o["ctr"][2] >= np.asarray(system["box"])[2, 1]
    p = run_product(script, system, tmp_path)
    one = results(p)
    p.close()
    session = uuid.uuid4().hex[:12]
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out.npz"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dd_indent_worker.py"), str(r), "2", session, sysfile, scriptfile, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    assert all(q.returncode == 0 for q in procs), "\n".join(logs)
    r = np.load(out)
    st, st1 = dict(zip(DD_STATS, r["stats"])), dict(zip(DD_STATS, one["stats"]))
    assert st["comm_nranks"] == 2 and 0 < st["nlocal"] < len(system["x"])
    for k in DD_STATS[:7]:
        assert st[k] == st1[k], (k, st[k], st1[k])
    assert st["steps_fused_indent"] == 43 and st["steps_unfused"] == 5
    for q in ("num_bond", "bond_type", "bond_atom", "type", "image", "f_loop", "f_loading", "f_unloading"):
        assert np.array_equal(r[q], one[q]), q
    print("2 slabs: x %.2e v %.2e rows %.2e indenter %.2e" % (np.abs(r["x"] - one["x"]).max(), np.abs(r["v"] - one["v"]).max(),
                                                              np.abs(r["rows"] - one["rows"]).max(), np.abs(r["indent"] - one["indent"]).max()))
    assert np.abs(r["x"] - one["x"]).max() < 1e-9
    assert np.abs(r["v"] - one["v"]).max() < 1e-8
    assert r["rows"].shape == one["rows"].shape and np.abs(r["rows"] - one["rows"]).max() < 1e-9
    assert abs(r["pe"][0] - one["pe"][0]) < 1e-9
    assert (np.abs(r["indent"] - one["indent"]) / np.maximum(1.0, np.abs(one["indent"]))).max() < 1e-9 and np.abs(one["indent"]).max() > 0
