"""Velocities handed from a rebuild to the step kernel (rebuild_plan.h RB_LAZY_V): k_permute leaves them in the old order
and the first launch of k_step after the build reads them through perm[] and stores them in the new one.

Every case runs the same job twice in fresh processes (lazy_permute_worker.py), as it comes and under
LAMMPS_LE_PERMUTE_ALL=1 (k_permute moves the velocities at every rebuild, as before), and asserts that the two runs agree
BIT FOR BIT after every `run` command: x, v, image, type by ID, the bond table, numneigh by ID, the owned IDs in list order,
the build positions, and the pair and bond entries of the list in list order; and that they rebuilt equally often.  Nothing
is recomputed, only moved, so any difference is a bug.  The throughput shape of the step kernel (one lane per bead, no
look-ahead - what a million beads take) is forced at these sizes with LAMMPS_LE_LPB=1 LAMMPS_LE_AHEAD_MAX_N=0; the bead
counts are no multiple of 64, the last wavefront is partial."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import le_state as ls
import neigh_inputs as I
from systems import CHAIN_SCRIPT, lattice_chain, wrap_into_box
from test_gpu_neigh import MINIMG_SCRIPT, SHAPES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LAZY_V = 1 << 26
SWITCH = "LAMMPS_LE_PERMUTE_ALL"
THROUGHPUT = SHAPES["throughput-shape"]
LIST_KEYS = ("owned", "xbuild", "itag", "jtag", "code", "btag", "bjtag", "btype")
SAME = ("x", "v", "image", "type", "numneigh") + LIST_KEYS + ("neigh_builds", "neigh_pairs", "maxneigh", "steps_fused",
                                                               "steps_fused_thermo", "steps_unfused")
# the fixes of the bench script (lammps_le_amd/synth.py CHAIN_INPUT), the LE fixes every 10 steps
BENCH_FIXES = """fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
fix loop all extrusion 10 1 1 1 1.0 2
fix loading all ex_load 10 1 1 1.12 2 prob 0.5 684474 iparam 1 1 jparam 1 1
fix unloading all ex_unload 10 2 0.5 prob 0.3 456456
"""
DELAY10 = MINIMG_SCRIPT.replace("neigh_modify every 1 delay 1 check yes", "neigh_modify every 1 delay 10 check yes")
EVERY_STEP = MINIMG_SCRIPT.replace("neigh_modify every 1 delay 1 check yes", "neigh_modify delay 0 every 1 check yes")
ALWAYS = MINIMG_SCRIPT.replace("neigh_modify every 1 delay 1 check yes", "neigh_modify delay 0 every 1 check no")
assert len({MINIMG_SCRIPT, DELAY10, EVERY_STEP, ALWAYS}) == 4


def crossing_chain():
    """4200 beads (65 wavefronts and 40 beads) in a 6.3 x 26.4 x 29.6 box, shifted so that the first lattice layer of every
    direction sits 0.08 from a periodic face: beads cross faces from the first steps on."""
    s = dict(I.rebuild_chain())
    s["x"] = s["x"] - 0.45
    s["x"], s["image"] = wrap_into_box(s)
    assert len(s["x"]) == 4200 and len(s["x"]) % 64
    return s


def run_job(tmp_path, label, system, actions, env):
    d = os.path.join(str(tmp_path), label)
    os.makedirs(d)
    jobfile, out = os.path.join(d, "job.pkl"), os.path.join(d, "out.npz")
    pickle.dump(dict(system=system, actions=actions), open(jobfile, "wb"))
    base = {k: v for k, v in os.environ.items() if k != SWITCH}
    p = subprocess.run([sys.executable, os.path.join(HERE, "lazy_permute_worker.py"), jobfile, out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=dict(base, **env), timeout=600)
    assert p.returncode == 0, p.stdout.decode()
    return dict(np.load(out))


def same_bits(a, b, keys, what):
    for key in keys:
        u, v = a[key], b[key]
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), "%s differs %s" % (key, what)


def twins(tmp_path, system, actions, env=None, label=""):
    """The job as it comes and under the switch; bit equality after every run command.  Returns (lazy run, permute-all run)."""
    env = dict(THROUGHPUT, **(env or {}))
    lazy = run_job(tmp_path, label + "lazy", system, actions, env)
    full = run_job(tmp_path, label + "all", system, actions, dict(env, **{SWITCH: "1"}))
    assert lazy["snapshots"][0] == full["snapshots"][0] >= 1
    for k in range(lazy["snapshots"][0]):
        same_bits(lazy, full, ["s%d_%s" % (k, key) for key in SAME], "between the two runs (run command %d)" % k)
        # under the switch no rebuild leaves the velocities behind; and in neither run was a stale order ever met:
        # settle_velocities is there for paths outside the time loop and launched nothing
        # ("rebuild_plan" is the plan without the new bit, what the hook with 22 facts answers; "rebuild_plan_full" has it)
        assert lazy["s%d_rebuild_plan" % k][0] == full["s%d_rebuild_plan" % k][0] == int(lazy["s%d_rebuild_plan_full" % k][0]) & ~LAZY_V
        assert full["s%d_lazy_rebuilds" % k][0] == 0 and not int(full["s%d_rebuild_plan_full" % k][0]) & LAZY_V
        assert lazy["s%d_velocities_settled" % k][0] == 0 and full["s%d_velocities_settled" % k][0] == 0
    same_bits(lazy, full, ("num_bond", "bond_type", "bond_atom"), "between the two runs")
    return lazy, full


def test_bench_fixes_in_a_small_box(tmp_path):
    """Case 1: `delay 10`, 80 steps: the displacement rebuilds and the ones the LE fixes force."""
    s = crossing_chain()
    lazy, _ = twins(tmp_path, s, [("script", DELAY10 + BENCH_FIXES + "run 80\n")])
    builds, took = lazy["s0_neigh_builds"][0], lazy["s0_lazy_rebuilds"][0]
    print("neigh_builds %d, of them lazy %d" % (builds, took))
    assert builds >= 5 and took >= 5
    assert (lazy["s0_image"] != s["image"]).any(axis=1).sum() >= 10, "no bead crossed a periodic face"
    assert lazy["bond_type"].max() == 2          # an extruder bond was loaded


def test_rebuild_follows_rebuild(tmp_path):
    """Case 2: `delay 0 every 1`: a rebuild may follow a rebuild, and the step after a build is itself a check-and-bin step -
    the launch that takes the velocities also bins."""
    s = crossing_chain()
    hot = BENCH_FIXES.replace("langevin 1.0 1.0", "langevin 4.0 4.0")
    lazy, _ = twins(tmp_path, s, [("script", EVERY_STEP + hot + "run 60\n")])
    builds, took = lazy["s0_neigh_builds"][0], lazy["s0_lazy_rebuilds"][0]
    print("neigh_builds %d, of them lazy %d" % (builds, took))
    assert builds >= 5 and took >= builds - 1          # (a rebuild on the last step of the run takes the old path)
    assert (lazy["s0_image"] != s["image"]).any()


def test_le_fixes_on_consecutive_steps(tmp_path):
    """Case 3: le_state's `wca-fene` input, 600 beads: extrusion / ex_unload / ex_load fire on consecutive steps of every
    10, each firing that changes the topology forces a rebuild one step after the last, with a topology snapshot."""
    s = ls.system_of("wca-fene")
    assert len(s["x"]) == 600 and len(s["x"]) % 64
    lazy, _ = twins(tmp_path, s, [("script", ls.script_of("wca-fene", 123))])
    builds = ls.oracle_end("wca-fene", 123)[0].neigh_builds()
    print("neigh_builds %d (oracle %d), of them lazy %d" % (lazy["s0_neigh_builds"][0], builds, lazy["s0_lazy_rebuilds"][0]))
    assert lazy["s0_neigh_builds"][0] == builds >= 3
    assert lazy["s0_lazy_rebuilds"][0] >= 3


def test_thermo_dump_and_last_steps_take_the_old_path(tmp_path):
    """Case 4: `delay 0 every 1 check no` rebuilds at every step, so rebuilds fall on thermo steps (every 7th), on dump steps
    (every 11th) and on the last step of the run: those take k_permute whole, every other one leaves the velocities."""
    s = crossing_chain()
    n = 40
    script = ALWAYS + BENCH_FIXES + "thermo 7\ndump 1 all custom 11 DUMPFILE id type x y z\nrun %d\n" % n
    lazy, _ = twins(tmp_path, s, [("script", script)])
    old_path = [t for t in range(1, n + 1) if t % 7 == 0 or t % 11 == 0 or t == n]
    assert lazy["s0_neigh_builds"][0] == n
    assert lazy["s0_lazy_rebuilds"][0] == n - len(old_path) > 0
    assert not int(lazy["s0_rebuild_plan_full"][0]) & LAZY_V          # the plan of the last step's rebuild
    # one step fewer: the run ends on a step that is neither a thermo nor a dump step, and is still the old path
    short, _ = twins(tmp_path, s, [("script", script.replace("run %d" % n, "run %d" % (n - 1)))], label="short-")
    assert (n - 1) % 7 and (n - 1) % 11
    assert short["s0_lazy_rebuilds"][0] == (n - 1) - len([t for t in old_path if t < n - 1]) - 1
    assert not int(short["s0_rebuild_plan_full"][0]) & LAZY_V


def test_overflow_right_after_a_lazy_rebuild(tmp_path):
    """Case 5: the table shrinks before the second build of the run; the step kernel behind it stores nothing, the host
    undoes the launch - the velocity hand-over with it -, grows the table, builds again and launches with the same arguments."""
    s = crossing_chain()
    lazy, _ = twins(tmp_path, s, [("script", DELAY10 + BENCH_FIXES + "run 40\n")], {"LAMMPS_LE_TEST_OVERFLOW_AT": "2"})
    assert lazy["s0_maxneigh"][0] > 4 and lazy["s0_lazy_rebuilds"][0] >= 3


def test_capi_and_restart_between_runs(tmp_path):
    """Case 6: two run commands with a C-ABI gather / scatter of v and image between them; then the same with a restart
    written after the scatter and read into a new instance - bit-continuous, as test_restart_is_bit_continuous asks."""
    s = crossing_chain()
    head = DELAY10 + BENCH_FIXES + "run 25\n"
    one = [("script", head), ("touch", None), ("script", "run 25\n")]
    two = [("script", head), ("touch", None), ("restart", BENCH_FIXES), ("script", "run 25\n")]
    a, a_all = twins(tmp_path, s, one, label="one-")
    b, _ = twins(tmp_path, s, two, label="two-")
    for r in (a, a_all, b):          # what was scattered is what came back, by ID
        same_bits(dict(u=r["touch_v"], w=r["touch_image"]), dict(u=r["touch_sent_v"], w=r["touch_sent_image"]), ("u", "w"), "after the scatter")
    assert (a["touch_image"] != a["s0_image"]).any() and (a["touch_v"] != a["s0_v"]).all()
    assert a["s1_lazy_rebuilds"][0] >= 1 and b["s1_lazy_rebuilds"][0] >= 1
    same_bits(a, b, ["s1_" + k for k in ("x", "v", "image", "type")] + ["num_bond", "bond_type", "bond_atom"], "between one instance and the restart")


def test_two_slabs_keep_the_old_path(tmp_path, monkeypatch):
    """Case 7: two z slabs in one process.  Decomposed rebuilds never leave the velocities behind, and the image flags are
    right after migration across the periodic z face: the 1-rank run's, exactly.  Positions and velocities: the decomposed
    suite holds either run within 1e-9 / 1e-8 of the same reference after these 60 steps (test_md_across_slabs: the ranks add
    a bead's pair terms in another list order), so the two are within twice that of each other."""
    from systems import run_product
    from test_gpu_dd import run_ranks_local
    n = 1500
    s = lattice_chain(n, nchains=2, seed=21)
    s["x"] = s["x"] - 0.45
    s["x"], s["image"] = wrap_into_box(s)
    assert n % 64
    script = CHAIN_SCRIPT.replace("comm_modify cutoff 5.0", "comm_modify cutoff 2.0") + \
        "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nthermo 30\nrun 60\n"
    for k, v in THROUGHPUT.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(SWITCH, raising=False)
    two = run_ranks_local(2, s, script, tmp_path, extra=lambda lmp: dict(lazy=np.array([lmp.stat("lazy_rebuilds")]),
                                                                         plan=np.array([lmp.stat("rebuild_plan_full")])))
    one = run_product(script, s, tmp_path)
    x, v, image = one.gather("x"), one.gather("v"), one.gather("image")
    assert two["lazy"][0] == 0 and not int(two["plan"][0]) & LAZY_V and one.stat("lazy_rebuilds") >= 3
    assert two["builds"][0] == one.stat("neigh_builds") >= 3
    one.close()
    crossed_z = image[:, 2] != s["image"][:, 2]
    print("beads that crossed the periodic z face: %d" % crossed_z.sum())
    assert crossed_z.sum() >= 3
    assert np.array_equal(two["image"], image)
    assert np.abs(two["x"] - x).max() < 2e-9 and np.abs(two["v"] - v).max() < 2e-8
