"""One run in a process of its own, for test_gpu_lazy_permute.py: the switches of the rebuild are read when a run starts, so
every configuration gets a fresh process.
usage: lazy_permute_worker.py JOB.pkl OUT.npz
JOB = dict(system=..., actions=[...]); an action is
  ("script", text)         the commands, line by line; after every `run` the state is recorded under the prefix "s<k>_"
  ("touch", None)          C-ABI between two runs: gather v and image, scatter them back shifted by a function of the ID
                           (v += 1e-3 sin(ID), the x image flag of every 7th ID += 1), gather again and record what came back
  ("restart", fixes)       write_restart, close the instance, read_restart into a new one, then the fix commands `fixes`
Recorded per `run`: x, v, image, type by ID; the list of the last build as the test hook hands it out (owned IDs in list
order, build positions, pair and bond entries in list order) and numneigh by ID counted from it; the stats."""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from neigh_worker import fetch_list

STATS = ("neigh_builds", "neigh_pairs", "rebuild_plan", "rebuild_plan_full", "lazy_rebuilds", "velocities_settled", "maxneigh", "steps_fused",
         "steps_fused_thermo", "steps_unfused")


def snapshot(lmp, res, k):
    for name in STATS:          # (first: the gathers below may settle nothing, but they are calls of their own)
        res["s%d_%s" % (k, name)] = np.array([lmp.stat(name)])
    L = fetch_list(lmp)
    for name, a in L.items():
        res["s%d_%s" % (k, name)] = a
    n = int(lmp.get_natoms())
    res["s%d_numneigh" % k] = np.bincount(L["itag"], minlength=n + 1) + np.bincount(L["btag"], minlength=n + 1)
    for name in ("x", "v", "image", "type"):
        res["s%d_%s" % (k, name)] = lmp.gather(name)


def main():
    from lammps_le_amd import lammps
    from systems import write_data
    jobfile, out = sys.argv[1], sys.argv[2]
    job = pickle.load(open(jobfile, "rb"))
    lmp = lammps(cmdargs=["-screen", "none"])
    res, k = {}, 0
    for kind, arg in job["actions"]:
        if kind == "touch":
            v, image = lmp.gather("v"), lmp.gather("image")
            ids = np.arange(1, len(v) + 1)
            v2, image2 = v + 1e-3 * np.sin(ids)[:, None], image.copy()
            image2[ids % 7 == 0, 0] += 1
            lmp.scatter("v", v2)
            lmp.scatter("image", image2)
            res["touch_v"], res["touch_image"] = lmp.gather("v"), lmp.gather("image")
            res["touch_sent_v"], res["touch_sent_image"] = v2, image2
            continue
        if kind == "restart":
            path = os.path.join(os.path.dirname(out), "state.restart")
            lmp.command("write_restart " + path)
            lmp.close()
            lmp = lammps(cmdargs=["-screen", "none"])
            lmp.command("read_restart " + path)
            for ln in arg.split("\n"):
                lmp.command(ln)
            continue
        for ln in arg.split("\n"):
            w = ln.split("#")[0].split()
            if w and w[0] == "read_data":
                path = os.path.join(os.path.dirname(out), "data.chain")
                write_data(path, job["system"])
                ln = "read_data " + path
            if w and w[0] == "dump":
                ln = ln.replace("DUMPFILE", os.path.join(os.path.dirname(out), "steps.dump"))
            lmp.command(ln)
            if w and w[0] == "run":
                snapshot(lmp, res, k)
                k += 1
    res["snapshots"] = np.array([k])
    for name in ("num_bond", "bond_type", "bond_atom"):
        res[name] = lmp.gather(name)
    np.savez(out, **res)
    lmp.close()


if __name__ == "__main__":
    main()
