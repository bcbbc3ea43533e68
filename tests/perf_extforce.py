"""Development probe: the default 1M-bead workload (scrambled start + the three LE fixes) with every 100th bead tethered
(fix spring/self 10.0) and an fix addforce on a second group of the same size:

  python tests/perf_extforce.py [NBEADS] [STEPS] [OUT.json]

After the usual pre-roll, three alternating pairs of runs of STEPS steps on one handle: the fixes inside the step kernel (its EXT
variant), and LAMMPS_LE_NO_FUSE=1 (k_fixforce behind the unfused kernels); then the two fixes are removed and three runs of the
default instantiation follow on the same handle.  Writes the rates and the step kernel's time per launch
(LAMMPS_LE_KERNEL_TIMING) to OUT.json (default profiles/extforce_walk1m.json) and prints the same as one JSON line.  The fused
variant has to beat the unfused path (exit status 1 if it does not); how much slower the EXT variant is than the default kernel
is reported, not judged."""
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
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "extforce_walk1m.json")
sysd = scrambled_chains(nbeads, nchains=1, seed=1, barrier_every=200)
data = os.path.join(tempfile.mkdtemp(prefix="le_extforce_"), "data")
write_data(data, sysd)
script = CHAIN_INPUT.format(data=data, n1=1000, left=2, right=3, tp=0.5, lr="4", nload=1000, pload=0.002, punload=0.05)
fixes = ("group teth id 100:%d:100\ngroup pull id 50:%d:100\nfix tether teth spring/self 10.0\nfix drift pull addforce 0.05 0.0 0.0\n"
         % (nbeads, nbeads))
os.environ["LAMMPS_LE_KERNEL_TIMING"] = "1"
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
lmp = lammps(cmdargs=["-screen", "none"])
for ln in (script + fixes).split("\n"):
    lmp.command(ln)
lmp.command("run 3010")
lmp.command("run 500")
rates, k_step_us, paths = dict(fused=[], unfused=[], without=[]), dict(fused=[], without=[]), {}
for rep in range(3):
    for mode in ("fused", "unfused"):
        if mode == "unfused":
            os.environ["LAMMPS_LE_NO_FUSE"] = "1"
        else:
            os.environ.pop("LAMMPS_LE_NO_FUSE", None)
        lmp.command("run %d" % steps)
        rates[mode].append(round(steps / lmp.stat("loop_time"), 1))
        paths[mode] = {k: int(lmp.stat(k)) for k in ("steps_fused", "steps_fused_ext", "steps_unfused")}
        if mode == "fused":
            k_step_us["fused"].append(round(1e3 * lmp.stat("pair_kernel_ms"), 2))
os.environ.pop("LAMMPS_LE_NO_FUSE", None)
spring_energy = lmp.extract_fix("tether", 0, 0)
lmp.command("unfix tether")
lmp.command("unfix drift")
for rep in range(3):
    lmp.command("run %d" % steps)
    rates["without"].append(round(steps / lmp.stat("loop_time"), 1))
    paths["without"] = {k: int(lmp.stat(k)) for k in ("steps_fused", "steps_fused_ext", "steps_unfused")}
    k_step_us["without"].append(round(1e3 * lmp.stat("pair_kernel_ms"), 2))
result = dict(beads=nbeads, steps=steps, members_per_fix=nbeads // 100, timesteps_per_s_fused=rates["fused"],
              timesteps_per_s_unfused=rates["unfused"], timesteps_per_s_without_the_fixes=rates["without"],
              k_step_us_ext=k_step_us["fused"], k_step_us_default=k_step_us["without"], paths=paths, spring_energy=spring_energy,
              builds_last_run=int(lmp.stat("neigh_builds")), bonds=int(lmp.get_thermo("bonds")), fene_warnings=int(lmp.stat("fene_warnings")))
lmp.close()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(result, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(result))
sys.exit(0 if min(rates["fused"]) > max(rates["unfused"]) else 1)
