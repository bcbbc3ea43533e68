"""One rank of a decomposed run that ends with the rows of local computes (test helper, launched by test_gpu_pair_rows.py).
usage: pair_rows_worker.py RANK WORLD SESSION SYSTEM.pkl SCRIPT.txt OUT ID[,ID...]   ->  OUT.rRANK.npz (rows_ID per compute, x,
host_downloads before and after the extracts)"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from lammps_le_amd import lammps
    from systems import write_data
    rank, world, session, sysfile, scriptfile, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    ids = sys.argv[7].split(",")
    system = pickle.load(open(sysfile, "rb"))
    lmp = lammps(cmdargs=["-screen", "none"])
    if world > 1:
        lmp.comm_init("shm", rank, world, session=session)
    for ln in open(scriptfile).read().split("\n"):
        w = ln.split("#")[0].split()
        if w and w[0] == "read_data":
            path = os.path.join(os.path.dirname(out), "data.r%d" % rank)
            write_data(path, system)
            ln = "read_data " + path
        lmp.command(ln)
    before = lmp.stat("host_downloads")
    res = {"rows_" + cid: lmp.pair_rows(cid) for cid in ids}          # (collective: every rank asks, every rank gets the whole table)
    after = lmp.stat("host_downloads")
    res.update(x=lmp.gather("x"), downloads=np.array([before, after]), nlocal=np.array([lmp.stat("nlocal")]))
    np.savez("%s.r%d.npz" % (out, rank), **res)
    lmp.close()


if __name__ == "__main__":
    main()
