"""One rank of a multi-process run of the decomposed engine with fix indent (test helper, launched by test_gpu_indent_dd.py; the
pattern of dd_extforce_worker.py, with the indenter's sums and the steps' paths in the result).
usage: dd_indent_worker.py RANK WORLD SESSION SYSTEM.pkl SCRIPT.txt OUT.npz"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lammps_le_amd import lammps
from systems import write_data

STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_indent", "neigh_builds",
         "fene_warnings", "comm_nranks", "nlocal")


def results(lmp):
    """What the one-rank run and every rank of a decomposed run report (gathers are collective: every rank calls them)."""
    res = dict(x=lmp.gather("x"), v=lmp.gather("v"), image=lmp.gather("image"), type=lmp.gather("type"),
               num_bond=lmp.gather("num_bond"), bond_type=lmp.gather("bond_type"), bond_atom=lmp.gather("bond_atom"),
               rows=np.asarray(lmp.thermo_history(), dtype=np.float64), pe=np.array([lmp.get_thermo("pe")]),
               indent=np.array([lmp.extract_fix("c", 0, 0)] + [lmp.extract_fix("c", 0, 1, k) for k in range(3)]),
               stats=np.array([lmp.stat(k) for k in STATS], dtype=np.float64))
    for fid in ("loop", "loading", "unloading"):
        res["f_" + fid] = np.array([lmp.extract_fix(fid, 0, 1, 0), lmp.extract_fix(fid, 0, 1, 1)])
    return res


if __name__ == "__main__":
    rank, world, session, sysfile, scriptfile, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    system = pickle.load(open(sysfile, "rb"))
    script = open(scriptfile).read()
    lmp = lammps(cmdargs=["-screen", "none"])
    lmp.comm_init("shm", rank, world, session=session)
    tmp = os.path.dirname(out)
    for ln in script.split("\n"):
        w = ln.split("#")[0].split()
        if w and w[0] == "read_data":
            path = os.path.join(tmp, "data.r%d" % rank)
            write_data(path, system)
            ln = "read_data " + path
        lmp.command(ln)
    res = results(lmp)
    if rank == 0:
        np.savez(out, **res)
    lmp.close()
