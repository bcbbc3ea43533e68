"""Development probe: what one force evaluation of `minimize` costs beside one thermo step of a run, on the same 1M-bead state
(the scrambled start of the default workload, no LE fixes: nve + langevin defined, silent in the minimisation):

  python tests/perf_minimize.py [NBEADS] [OUT.json]

Three alternating pairs on one handle: `minimize 0 0 50 100000` - wall time of its loop per force evaluation - and a 50-step
`run` with `thermo 1`, which takes the same unfused energy-evaluating kernels on every step - wall time of its loop per step.
Writes both, their ratio, the evaluation and wait counts to OUT.json (default profiles/minimize_walk1m.json) and prints the same."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lammps_le_amd import lammps
from lammps_le_amd.synth import scrambled_chains, write_data

nbeads = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "minimize_walk1m.json")
data = os.path.join(tempfile.mkdtemp(prefix="le_min_"), "data")
write_data(data, scrambled_chains(nbeads, nchains=1, seed=1, barrier_every=200))
HEAD = """units lj
atom_style bond
newton off
atom_modify sort 0 0
special_bonds fene
read_data %s
neighbor 0.4 bin
neigh_modify every 1 delay 0 check yes
bond_style fene
bond_coeff 1 30.0 1.5 1.0 1.0
bond_coeff 2 30.0 4.0 1.0 1.0
timestep 0.005
pair_style lj/cut 1.12
pair_modify shift yes
pair_coeff * * 1.0 1.0 1.12
fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
""" % data
lmp = lammps(cmdargs=["-screen", "none"])
for ln in HEAD.split("\n"):
    lmp.command(ln)
rows = dict(eval_us=[], thermo_step_us=[], evals=[], iterations=[], host_waits=[], rebuilds=[], stop=[])
for rep in range(3):
    lmp.command("thermo 10")
    res = lmp.minimize(0.0, 0.0, 50, 100000)
    rows["eval_us"].append(round(1e6 * lmp.stat("loop_time") / max(res["evals"], 1), 2))
    rows["evals"].append(res["evals"])
    rows["iterations"].append(res["iterations"])
    rows["stop"].append(res["stop"])
    rows["host_waits"].append(int(lmp.stat("min_host_waits")))
    rows["rebuilds"].append(int(lmp.stat("min_rebuilds")))
    lmp.command("thermo 1")
    lmp.command("run 50")
    rows["thermo_step_us"].append(round(1e6 * lmp.stat("loop_time") / 50, 2))
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
result = dict(beads=nbeads, ratio_eval_over_thermo_step=round(med(rows["eval_us"]) / med(rows["thermo_step_us"]), 3),
              fene_warnings=int(lmp.stat("fene_warnings")), **rows)
lmp.close()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(result, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(result))
