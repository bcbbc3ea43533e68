"""One rank of a run in a process of its own, for test_gpu_rebuild_chain.py: the switches of the rebuild are read when a run
starts and the layout is allocated once per handle, so every library configuration gets a fresh process.
usage: rebuild_chain_worker.py RANK WORLD SESSION JOB.pkl OUT   ->  OUT.rRANK.npz
JOB = dict(system=..., actions=[("script", text) | ("scatter_x", amplitude) | ("snapshot", None), ...]).  After every `run` command of a script
action the state is recorded under the prefix "s<k>_": x, v, image by tag, and the neighbor list of the last build as the
test hook hands it out (owned tags in list order, the build positions xhold, pair and bond entries in list order)."""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from neigh_worker import fetch_list


def snapshot(lmp, res, k):
    L = fetch_list(lmp)
    for name, a in L.items():
        res["s%d_%s" % (k, name)] = a
    for name in ("x", "v", "image"):          # (collective: every rank calls them)
        res["s%d_%s" % (k, name)] = lmp.gather(name)
    for name in ("neigh_builds", "neigh_pairs", "rebuild_plan", "maxneigh", "special_asym"):
        res["s%d_%s" % (k, name)] = np.array([lmp.stat(name)])


def main():
    from lammps_le_amd import lammps
    from systems import write_data
    rank, world, session, jobfile, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    job = pickle.load(open(jobfile, "rb"))
    lmp = lammps(cmdargs=["-screen", "none"])
    if world > 1:
        lmp.comm_init("shm", rank, world, session=session)
    res, k = {}, 0
    for kind, arg in job["actions"]:
        if kind == "scatter_x":          # every bead nudged by a smooth function of its tag, through the C-ABI
            x = lmp.gather("x")
            t = np.arange(1, len(x) + 1, dtype=np.float64)
            lmp.scatter("x", x + arg * np.stack([np.sin(t), np.cos(2.0 * t), np.sin(3.0 * t)], axis=1))
            continue
        if kind == "snapshot":          # (between two run commands: the list and xhold of the last build, the state as it is now)
            snapshot(lmp, res, k)
            k += 1
            continue
        for ln in arg.split("\n"):
            w = ln.split("#")[0].split()
            if w and w[0] == "read_data":
                path = os.path.join(os.path.dirname(out), "data.r%d" % rank)
                write_data(path, job["system"])
                ln = "read_data " + path
            lmp.command(ln)
            if w and w[0] == "run":
                snapshot(lmp, res, k)
                k += 1
    res["snapshots"] = np.array([k])
    for name in ("num_bond", "bond_type", "bond_atom"):
        res[name] = lmp.gather(name)
    res["bond_minimg"] = np.array([lmp.stat("bond_minimg")])
    np.savez("%s.r%d.npz" % (out, rank), **res)
    lmp.close()


if __name__ == "__main__":
    main()
