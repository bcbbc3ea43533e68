"""Development probe: the default 1M-bead workload (scrambled start + the three LE fixes) confined by fix wall/region - the data
file's box widened by 2 sigma per side, a lj126 block wall (cutoff 2^(1/6): WCA) 0.6 sigma outside the lattice's cube, so that no
bead starts inside the cutoff:

  python tests/perf_wall.py [NBEADS] [STEPS] [OUT.json]

After the usual pre-roll, three alternating pairs of runs of STEPS steps on one handle: the wall inside the step kernel (its
wall variant), and LAMMPS_LE_NO_FUSE=1 (k_wall behind the unfused kernels).  Writes the rates, their ranges and the step
kernel's time (LAMMPS_LE_KERNEL_TIMING) to OUT.json (default profiles/wall_walk1m.json) and prints the same as one JSON line."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lammps_le_amd import lammps
from lammps_le_amd.synth import CHAIN_INPUT, scrambled_chains, write_data

nbeads = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "wall_walk1m.json")
sysd = scrambled_chains(nbeads, nchains=1, seed=1, barrier_every=200)
cube = [(float(lo), float(hi)) for lo, hi in sysd["box"]]
sysd["box"] = [(lo - 2.0, hi + 2.0) for lo, hi in cube]
data = os.path.join(tempfile.mkdtemp(prefix="le_wall_"), "data")
write_data(data, sysd)
script = CHAIN_INPUT.format(data=data, n1=1000, left=2, right=3, tp=0.5, lr="4", nload=1000, pload=0.002, punload=0.05)
wall = "region cube block " + " ".join("%.17g %.17g" % (lo - 0.6, hi + 0.6) for lo, hi in cube) + \
       "\nfix wall all wall/region cube lj126 1.0 1.0 1.122462048309373\n"
os.environ["LAMMPS_LE_KERNEL_TIMING"] = "1"
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
lmp = lammps(cmdargs=["-screen", "none"])
for ln in (script + wall).split("\n"):
    lmp.command(ln)
lmp.command("run 3010")
lmp.command("run 500")
rates, k_step_us, paths = dict(fused=[], unfused=[]), [], {}
for rep in range(3):
    for mode in ("fused", "unfused"):
        if mode == "unfused":
            os.environ["LAMMPS_LE_NO_FUSE"] = "1"
        else:
            os.environ.pop("LAMMPS_LE_NO_FUSE", None)
        lmp.command("run %d" % steps)
        rates[mode].append(round(steps / lmp.stat("loop_time"), 1))
        paths[mode] = {k: int(lmp.stat(k)) for k in ("steps_fused", "steps_fused_wall", "steps_unfused")}
        if mode == "fused":
            k_step_us.append(round(1e3 * lmp.stat("pair_kernel_ms"), 2))
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
result = dict(beads=nbeads, steps=steps, timesteps_per_s_fused=rates["fused"], timesteps_per_s_unfused=rates["unfused"],
              k_step_us_fused=k_step_us, paths=paths, wall_energy=lmp.extract_fix("wall", 0, 0), builds_last_run=int(lmp.stat("neigh_builds")),
              bonds=int(lmp.get_thermo("bonds")), fene_warnings=int(lmp.stat("fene_warnings")))
lmp.close()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(result, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(result))
