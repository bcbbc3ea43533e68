"""One rank of a two-slab run that names fmax / fnorm in its thermo line and then asks for a minimisation (test helper, launched
by test_gpu_minimize.py; the pattern of dd_extforce_worker.py).
usage: dd_minimize_worker.py RANK WORLD SESSION SYSTEM.pkl SCRIPT.txt OUT.npz"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lammps_le_amd import lammps
from systems import write_data


def results(lmp):
    """fmax / fnorm of the last thermo row beside the gathered forces, then the refusal of `minimize` on a decomposed handle
    (every rank refuses before anything collective starts) and a run behind it.  On one GPU the minimisation is not tried."""
    res = dict(fmax=np.array([lmp.get_thermo("fmax")]), fnorm=np.array([lmp.get_thermo("fnorm")]), f=lmp.gather("f"),
               nranks=np.array([lmp.stat("comm_nranks")]), nlocal=np.array([lmp.stat("nlocal")]))
    text = ""
    if res["nranks"][0] > 1:
        try:
            lmp.command("minimize 0 0 5 100")
        except Exception as e:          # noqa: BLE001
            text = str(e)
        lmp.command("run 5")
    res["refusal"] = np.array([text])
    res["step"] = np.array([lmp.get_thermo("step")])
    res["fmax_after"] = np.array([lmp.get_thermo("fmax")])
    res["f_after"] = lmp.gather("f")
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
