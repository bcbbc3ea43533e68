"""Development probe: what the soft variant of the step kernel costs beside the lj/cut variant, on the same 1M-bead state (the
scrambled start of the default workload, no LE fixes: nve + langevin), and what fix adapt adds per step:

  python tests/perf_soft.py [NBEADS] [STEPS] [OUT.json]

After a pre-roll under lj/cut, three alternating pairs of runs of STEPS steps on one handle - pair_style soft 1.12246 with A = 30
and pair_style lj/cut 1.12 -, each with the step kernel's own begin / end timestamps (LAMMPS_LE_KERNEL_TIMING); then soft with
`fix adapt 1 ... v_A` (A constant, so that the state stays comparable) against `fix adapt 0`, with one coefficient set (the
launch's scalars carry the value) and with a second set on the barrier types (the table is copied every step).  Writes the kernel times,
their ratio, the rates and the per-step cost of adapt 1 to OUT.json (default profiles/soft_walk1m.json) and prints the same."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lammps_le_amd import lammps
from lammps_le_amd.synth import scrambled_chains, write_data

nbeads = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "soft_walk1m.json")
data = os.path.join(tempfile.mkdtemp(prefix="le_soft_"), "data")
write_data(data, scrambled_chains(nbeads, nchains=1, seed=1, barrier_every=200))
HEAD = """units lj
atom_style bond
newton off
atom_modify sort 0 0
special_bonds fene
read_data %s
neighbor 0.4 bin
neigh_modify every 1 delay 10 check yes
bond_style fene
bond_coeff 1 30.0 1.5 1.0 1.0
bond_coeff 2 30.0 4.0 1.0 1.0
timestep 0.005
fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
""" % data
LJ = "pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12"
SOFT = "pair_style soft 1.12246\npair_coeff * * 30.0"
os.environ["LAMMPS_LE_KERNEL_TIMING"] = "1"
lmp = lammps(cmdargs=["-screen", "none"])


def cmds(text):
    for ln in text.split("\n"):
        lmp.command(ln)


def run():
    lmp.command("run %d" % steps)
    return round(steps / lmp.stat("loop_time"), 1), round(1e3 * lmp.stat("pair_kernel_ms"), 2), int(lmp.stat("steps_fused_soft"))


cmds(HEAD + LJ)
lmp.command("run 1000")
rate, kus, soft_steps = dict(soft=[], lj=[]), dict(soft=[], lj=[]), 0
for rep in range(3):
    for mode, style in (("soft", SOFT), ("lj", LJ)):
        cmds(style)
        r, k, n = run()
        rate[mode].append(r)
        kus[mode].append(k)
        soft_steps = max(soft_steps, n)
adapt = {}
lmp.command("variable A equal 30.0")
for label, coeffs, pairs in (("scalars", SOFT, "* *"), ("table", SOFT + "\npair_coeff 2*4 2*4 29.0", "1 1")):
    cmds(coeffs)
    rows = {}
    for every in (0, 1, 0, 1):
        lmp.command("fix push all adapt %d pair soft a %s v_A" % (every, pairs))
        copies0 = lmp.stat("pair_table_copies")
        r, k, n = run()
        rows.setdefault("adapt%d" % every, []).append(r)
        rows["table_copies_adapt%d" % every] = int(lmp.stat("pair_table_copies") - copies0)
        lmp.command("unfix push")
    a0, a1 = max(rows["adapt0"]), max(rows["adapt1"])
    rows["adapt1_cost_us_per_step"] = round(1e6 * (1.0 / a1 - 1.0 / a0), 3)
    adapt[label] = rows
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
result = dict(beads=nbeads, steps=steps, k_step_us_soft=kus["soft"], k_step_us_lj=kus["lj"], k_step_ratio_soft_over_lj=round(med(kus["soft"]) / med(kus["lj"]), 3),
              timesteps_per_s_soft=rate["soft"], timesteps_per_s_lj=rate["lj"], steps_fused_soft=soft_steps, adapt=adapt,
              fene_warnings=int(lmp.stat("fene_warnings")))
lmp.close()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(result, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(result))
