"""Development probe: the default 1M-bead workload (scrambled start + the three LE fixes) inside a sphere-in fix indent whose
radius is a formula of the step - the data file's box widened by 2 sigma per side, R = ramp(far + 2.0, far + 0.6) with `far` the
distance of the farthest bead of the start from the centre, so that the indenter never touches a bead and the physics stays the
benchmark's while every launch carries the table and every bead runs indent_force:

  python tests/perf_indent.py [NBEADS] [STEPS] [OUT.json]

After the usual pre-roll, three alternating pairs of runs of STEPS steps on one handle: the indenter inside the step kernel (its
indent variant), and LAMMPS_LE_NO_FUSE=1 (k_indent behind the unfused kernels).  Writes the rates, their ranges and the step
kernel's time (LAMMPS_LE_KERNEL_TIMING) to OUT.json (default profiles/indent_walk1m.json) and prints the same as one JSON line.
An OUT.json that already holds `guards` keeps them.

  python tests/perf_indent.py guards DIR [OUT.json]

writes that block: the two comparisons against the parent commit the issue asks for, from the outputs of runs on one GPU in one
session, alternating, which DIR holds - `bench_parent_K.json` / `bench_this_K.json` (K = 1 2 3; the JSON line of `python bench.py
--gpus 1 --steps 2000 --warmup 500` in a checkout of the parent and in this one) and `wall_parent_K.json` / `wall_this_K.json`
(K = 1 2 ..; the output files of `python tests/perf_wall.py 1000000 2000 FILE`).  A guard holds when this commit's mean is below
the parent's by at most three times the range of the parent's three repetitions."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lammps_le_amd import lammps
from lammps_le_amd.synth import CHAIN_INPUT, scrambled_chains, write_data



def write_guards(src, out):
    import glob

    def load(pattern, key):
        return [json.load(open(f))[key] for f in sorted(glob.glob(os.path.join(src, pattern)))]

    def spread(v):
        return round(max(v) - min(v), 1)

    def mean(v):
        return sum(v) / len(v)
    bp, bt = load("bench_parent_*.json", "value"), load("bench_this_*.json", "value")
    wp, wt = load("wall_parent_*.json", "timesteps_per_s_fused"), load("wall_this_*.json", "timesteps_per_s_fused")
    kp, kt = load("wall_parent_*.json", "k_step_us_fused"), load("wall_this_*.json", "k_step_us_fused")
    assert len(bp) == len(bt) == 3 and len(wp) == len(wt) >= 1
    wall_range = spread(wp[0])
    wall_deficit = mean([x for r in wp for x in r]) - mean([x for r in wt for x in r])
    guards = dict(
        note="the parent commit and this one on the same MI355X in one session, alternating; allowed: slower than the parent by at most "
             "three times the range of the parent's three repetitions",
        bench=dict(command="python bench.py --gpus 1 --steps 2000 --warmup 500", parent_timesteps_per_s=bp, this_timesteps_per_s=bt,
                   parent_range=spread(bp), allowed_deficit=round(3 * spread(bp), 1), deficit_of_means=round(mean(bp) - mean(bt), 1),
                   holds=bool(mean(bp) - mean(bt) <= 3 * spread(bp))),
        perf_wall=dict(command="python tests/perf_wall.py 1000000 2000", parent_timesteps_per_s_fused=wp, this_timesteps_per_s_fused=wt,
                       parent_k_step_us=kp, this_k_step_us=kt, parent_range=wall_range, allowed_deficit=round(3 * wall_range, 1),
                       deficit_of_means=round(wall_deficit, 1), holds=bool(wall_deficit <= 3 * wall_range)))
    result = json.load(open(out)) if os.path.exists(out) else {}
    result["guards"] = guards
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(guards))


if len(sys.argv) > 2 and sys.argv[1] == "guards":
    write_guards(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "indent_walk1m.json"))
    sys.exit(0)

nbeads = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "indent_walk1m.json")
sysd = scrambled_chains(nbeads, nchains=1, seed=1, barrier_every=200)
cube = [(float(lo), float(hi)) for lo, hi in sysd["box"]]
sysd["box"] = [(lo - 2.0, hi + 2.0) for lo, hi in cube]
centre = [0.5 * (lo + hi) for lo, hi in cube]
far = float(np.sqrt(((np.asarray(sysd["x"], dtype=np.float64) - np.asarray(centre)[None, :]) ** 2).sum(axis=1)).max())
data = os.path.join(tempfile.mkdtemp(prefix="le_indent_"), "data")
write_data(data, sysd)
script = CHAIN_INPUT.format(data=data, n1=1000, left=2, right=3, tp=0.5, lr="4", nload=1000, pload=0.002, punload=0.05)
indent = "variable R equal ramp(%.17g,%.17g)\nfix c all indent 10.0 sphere %.17g %.17g %.17g v_R side in units box\n" % (
    far + 2.0, far + 0.6, centre[0], centre[1], centre[2])
os.environ["LAMMPS_LE_KERNEL_TIMING"] = "1"
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
lmp = lammps(cmdargs=["-screen", "none"])
for ln in (script + indent).split("\n"):
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
        paths[mode] = {k: int(lmp.stat(k)) for k in ("steps_fused", "steps_fused_indent", "steps_fused_wall", "steps_unfused")}
        if mode == "fused":
            k_step_us.append(round(1e3 * lmp.stat("pair_kernel_ms"), 2))
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
result = dict(beads=nbeads, steps=steps, timesteps_per_s_fused=rates["fused"], timesteps_per_s_unfused=rates["unfused"],
              k_step_us_fused=k_step_us, paths=paths, indenter_energy=lmp.extract_fix("c", 0, 0), farthest_bead=far,
              builds_last_run=int(lmp.stat("neigh_builds")), bonds=int(lmp.get_thermo("bonds")), fene_warnings=int(lmp.stat("fene_warnings")))
lmp.close()
if os.path.exists(out):
    try:
        old = json.load(open(out))
        if "guards" in old:
            result["guards"] = old["guards"]
    except ValueError:
        pass
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(result, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(result))
