"""The scenario table of the recorded reference runs (tests/golden/ref_*.npz) and the one comparison every side goes through.

A scenario is a start system, the script text that the oracle, the engine and the reference binary all run, the checkpoint
steps, and the lines the reference needs on top to write its state out (record_lines: its thermo columns, the local computes
behind the bond and angle rows, the dumps).  tests/golden/make_reference_runs.py runs the reference on each and stores numbers
only; test_reference_runs_cpu.py holds the oracle to them, test_gpu_reference_runs.py the HIP path.  This module needs neither
torch nor a device.

Every start is a melt: the reference itself ran nve + Langevin for MELT_STEPS steps from the lattice start of
systems.lattice_chain and the state it wrote is the stored start (ref_melt_*.npz, shared among scenarios); the melt itself is
compared with nothing.  Types are laid over the melted coordinates afterwards.
"""
import os

import numpy as np

from systems import ANGLE_SCRIPT, CHAIN_SCRIPT, barrier_types, lattice_chain, le_script

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MELT_STEPS = 1500
FACTOR = 16.0                    # README: the oracle against the brute force; here against the reference's own spread
# thermo columns the reference records (after `step`), then two vector entries per LE fix
THERMO = ("temp", "epair", "emol", "etotal", "press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz", "bonds", "angles")
RANMARS_SEEDS = (12345, 904297, 684474, 456456, 1, 900000000)
RANMARS_BEADS, RANMARS_RUNS = 1112, 3


# ------------------------------------------------------------------------------------------------------------------
# systems
# ------------------------------------------------------------------------------------------------------------------
def melt_key(n, nchains, seed):
    return "n%d_c%d_s%d" % (n, nchains, seed)


def melt_script(seed):
    return CHAIN_SCRIPT + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 %d\nrun %d\n" % (777 + seed, MELT_STEPS)


def lattice_start(n, nchains, seed):
    s = lattice_chain(n, nchains=nchains, seed=seed)
    s["ntypes"], s["mass"] = 4, [1.0] * 4          # every type a fix extrusion line may name exists in the file
    return s


def load_melt(n, nchains, seed):
    """The melted start as the reference wrote it."""
    s = lattice_start(n, nchains, seed)
    with np.load(os.path.join(GOLDEN, "ref_melt_%s.npz" % melt_key(n, nchains, seed))) as z:
        s["x"], s["v"], s["image"] = z["x"].copy(), z["v"].copy(), z["image"].copy()
    return s


def sticky_types(n, seed=3, frac=0.3):
    return np.where(np.random.RandomState(seed).rand(n) < frac, 2, 1).astype(np.int32)


def anchored_types(n, seed):
    """Barrier beads of types 2 and 3 as in barrier_types, and every type-4 bead an anchor (outside the group `mobile`)."""
    return barrier_types(n, seed, frac=0.3)


def build_system(scn, melt=None, recorded=None):
    """The start system of a scenario; melt = a loaded melt (the generator passes the one it has just made).  recorded: the
    arrays of the scenario's fixture - the types and the order of the Atoms section are then the recorded ones, not drawn
    again (the tests go this way: what they run does not depend on a random stream giving the same numbers for ever)."""
    p = scn["system"]
    n, nchains, seed = p["n"], p.get("nchains", 1), p.get("seed", 1)
    s = dict(melt) if melt is not None else load_melt(n, nchains, seed)
    if p.get("rows_along_z"):          # lattice_chain lays the chain in rows along x and a melt keeps that: exchange x and z
        for k in ("x", "v", "image"):  # (cubic box), so that extruder bonds reach across the faces between z slabs
            s[k] = np.ascontiguousarray(np.asarray(s[k])[:, ::-1])
    if recorded is not None:
        s["type"] = recorded["start_type"].copy()
    elif p.get("types") is not None:
        kind, a = p["types"][0], p["types"][1:]
        s["type"] = {"barrier": barrier_types, "sticky": sticky_types, "anchored": anchored_types}[kind](n, *a)
    if recorded is not None and "start_file_order" in recorded:
        s["file_order"] = recorded["start_file_order"].astype(np.int64)
    elif p.get("file_order") is not None:
        s["file_order"] = np.random.RandomState(p["file_order"]).permutation(n)
    if p.get("angles"):
        per = n // nchains
        ang = [(1, i, i + 1, i + 2) for i in range(1, n - 1) if (i - 1) // per == (i + 1) // per]
        s["nangletypes"], s["angles"], s["extra_angle"] = 2, np.array(ang, dtype=np.int32), 24
        s["atom_style"] = "molecular"
    # the capacities of the limit scenarios and their twins (the `extra ... per atom` lines of the data file), extruder bonds
    # the data file already holds (rows (a, b) of type 2), and single beads given another type
    for k in ("extra_bond", "extra_special", "extra_angle"):
        if k in p:
            s[k] = p[k]
    if p.get("ext_bonds"):
        s["bonds"] = np.concatenate([s["bonds"], np.array([(2, a, b) for a, b in p["ext_bonds"]], dtype=np.int32)])
    if p.get("type_at") and recorded is None:
        s["type"] = np.array(s["type"], dtype=np.int32)
        for tag, t in p["type_at"]:
            s["type"][tag - 1] = t
    return s


def ranmars_system():
    """RANMARS_BEADS free beads on a 2.0 grid (no pair within 1.12, no bonds), zero velocities: with v = 0 the force after
    `run 0` is the Langevin draw alone, sqrt(24 / dt) (u - 0.5)."""
    n, L = RANMARS_BEADS, 11
    k = np.arange(n)
    x = np.stack([k % L, (k // L) % L, k // (L * L)], axis=1).astype(np.float64) * 2.0 + 1.0
    return dict(box=np.array([[0.0, 2.0 * L]] * 3), x=x, v=np.zeros((n, 3)), type=np.ones(n, dtype=np.int32),
                mol=np.ones(n, dtype=np.int32), image=np.zeros((n, 3), dtype=np.int32), bonds=np.zeros((0, 3), dtype=np.int32),
                ntypes=1, nbondtypes=2, mass=[1.0], extra_bond=1, extra_special=20, atom_style="bond")


def ranmars_script(seed):
    return CHAIN_SCRIPT + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 %d\n" % seed


RANMARS_SCALE = np.sqrt(24.0 / 0.005)          # fix_langevin: sqrt(24 kT m / (dt damp)) at kT = m = damp = 1, dt = 0.005


def draws_from_forces(f):
    """Forces of a bead set at rest -> the 24-bit integers behind the uniform draws, in local order x, y, z; and how far from
    an integer the worst one sits (the read-out is exact when that is ~1e-9)."""
    u = (np.asarray(f, dtype=np.float64).reshape(-1) / RANMARS_SCALE + 0.5) * 16777216.0
    k = np.rint(u)
    return k.astype(np.int64), float(np.abs(u - k).max())


# ------------------------------------------------------------------------------------------------------------------
# scenarios
# ------------------------------------------------------------------------------------------------------------------
N = 1000
BAR = dict(n=N, types=("barrier", 5, 0.3))
LE3 = ("loop", "loading", "unloading")
_CYCLE = dict(n1=4, nl=5, nu=6)
STOCK = CHAIN_SCRIPT.replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 5.0 10.0 1.0 1.0") + (
    "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\n"
    "fix creating all bond/create 5 2 2 1.1 2 iparam 1 3 jparam 1 3 %s\n"
    "fix breaking all bond/break 6 2 1.3 prob 0.5 2211\nthermo 10\n")
ANGLES = ANGLE_SCRIPT + """angle_style %s
angle_coeff 1 %s
angle_coeff 2 %s
fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
fix loop all extrusion 7 1 1 1 1.0 2
fix loading all ex_load 5 1 1 1.12 2 prob 0.3 684474 iparam 1 1 jparam 1 1 atype 2
fix unloading all ex_unload 6 2 0.5 prob 0.4 456456
thermo 16
"""
_GROUP = le_script(tp=0.5, **_CYCLE).replace("fix 1 all nve", "group mobile type 1 2 3\nfix 1 mobile nve") \
    .replace("fix 2 all langevin", "fix 2 mobile langevin").replace("fix loop all", "fix loop mobile") \
    .replace("fix loading all", "fix loading mobile").replace("fix unloading all", "fix unloading mobile")


# 2 and 3 z slabs of 2048 beads (box 13.4) admit a ghost cutoff of at most 3.3 (device.h slab_rule), and on several ranks a
# bond must stay inside it: the stiff extruder bond of CHAIN_SCRIPT (30.0 4.0), and an ex_unload without `prob` that takes
# every extruder bond longer than 2.0 away every 4 steps (reached(): along_z holds the longest one over all steps to 3.0)
_DD = le_script(tp=0.5, n1=10, nl=5, nu=4, lprob="prob 0.9 684474", uprob="", rmax=2.0) \
    .replace("comm_modify cutoff 5.0", "comm_modify cutoff 3.3").replace("bond_coeff 2 5.0 10.0 1.0 1.0", "bond_coeff 2 30.0 4.0 1.0 1.0")
_SLABS = dict(n=2048, seed=4, types=("barrier", 5, 0.3), rows_along_z=True)


def _scn(name, system, script, steps=64, mid=None, fixes=LE3, family=None, contrast=None, point="", min_ext=5, idle=()):
    """steps: the last checkpoint (the sum of the script's run commands); mid: one earlier checkpoint, recorded in full, for
    the scenarios the GPU suite follows step-wise; contrast: (old, new) text - the reference run with old replaced by new must
    end in other bond rows (or another state): how the generator tells that the scenario's rule was reached; point: a named
    check on the recorded run itself (reached()); idle: fixes that must NOT have acted in the reference (condition (c) asks
    every other one to have acted)."""
    return dict(name=name, system=system, script=script, checkpoints=([mid] if mid else []) + [steps], fixes=fixes,
                family=family, contrast=contrast, point=point, min_ext=min_ext, idle=idle)


def _sorted(script, period):
    return script.replace("atom_modify sort 0 0", "atom_modify sort %d 0" % period)


SCENARIOS = [
    # left / right / roadblock barriers at the three through probabilities; 30 % barrier beads of types 2, 3, 4
    _scn("cycle_tp0", BAR, le_script(tp=0.0, **_CYCLE) + "run 64\n", contrast=("1 2 3 0.0 2 4", "1 2 3 1.0 2 4")),
    _scn("cycle_tp05", BAR, le_script(tp=0.5, **_CYCLE) + "run 64\n", mid=32, family="cycle", contrast=("1 2 3 0.5 2 4", "1 2 3 1.0 2 4")),
    _scn("cycle_tp1", BAR, le_script(tp=1.0, **_CYCLE) + "run 64\n", contrast=("1 2 3 1.0 2 4", "1 2 3 0.0 2 4")),
    _scn("no_roadblock", BAR, le_script(tp=0.5, lr="", **_CYCLE) + "run 64\n", contrast=("0.5 2 \n", "0.5 2 4\n")),
    # the roadblock type is a barrier type: two draws on one bead, the second only after the first let it through
    _scn("roadblock_is_left", BAR, le_script(tp=0.5, lr="2", **_CYCLE) + "run 64\n", contrast=("0.5 2 2\n", "0.5 2 4\n")),
    _scn("roadblock_is_right", BAR, le_script(tp=0.7, lr="3", **_CYCLE) + "run 64\n", contrast=("0.7 2 3\n", "0.7 2 4\n")),
    # every eligible (i, i+2) pair loads: runs of adjacent candidates, collisions, stalled extruders; four chains
    _scn("dense", dict(n=N, nchains=4, seed=2), le_script(n1=5, nl=10, nu=9, left=1, right=1, lprob="", uprob="prob 0.05 456456", lr="",
                                                          rmax=0.5) + "run 60\n", steps=60, point="stall", min_ext=50),
    _scn("chains4", dict(n=N, nchains=4, seed=2, types=("barrier", 7, 0.15)), le_script(tp=0.5, **_CYCLE) + "run 64\n", point="chains"),
    _scn("straddle", dict(n=N, seed=3, types=("barrier", 9, 0.3)),
         le_script(n1=4, nl=8, nu=8, tp=0.5, lprob="prob 0.8 684474", uprob="prob 0.2 456456", rmax=1.5) + "run 72\n", steps=72, point="straddle"),
    # Atom::sort: one period shorter than every fix period (4, 5, 6), one longer than all of them
    _scn("sort3", BAR, _sorted(le_script(tp=0.5, **_CYCLE), 3) + "run 64\n", mid=32, family="sort",
         contrast=("atom_modify sort 3 0", "atom_modify sort 0 0"), point="sorted"),
    _scn("sort7", BAR, _sorted(le_script(tp=0.0, **_CYCLE), 7) + "run 64\n", contrast=("atom_modify sort 7 0", "atom_modify sort 0 0"),
         point="sorted"),
    _scn("file_order", dict(n=N, file_order=5), le_script(left=1, right=1, lr="", **_CYCLE) + "run 48\n", steps=48, point="file_order"),
    _scn("newton_on", dict(n=N, types=("barrier", 17, 0.3)),
         le_script(lprob="prob 0.8 684474", **_CYCLE).replace("newton off", "newton on off") + "run 48\n", steps=48,
         contrast=("newton on off", "newton off")),
    _scn("newton_on_sort9", dict(n=N, types=("barrier", 17, 0.3)),
         _sorted(le_script(lprob="prob 0.8 684474", **_CYCLE).replace("newton off", "newton on off"), 9) + "run 48\n", steps=48,
         contrast=("atom_modify sort 9 0", "atom_modify sort 0 0"), point="sorted"),
    # src/MC parents
    _scn("stock_create", dict(n=N, types=("sticky",)), STOCK % "" + "run 60\n", steps=60, fixes=("creating", "breaking"), family="stock",
         mid=30, point="stock"),
    _scn("stock_create_prob", dict(n=N, types=("sticky",)), STOCK % "prob 0.5 8847" + "run 60\n", steps=60, fixes=("creating", "breaking"),
         contrast=("prob 0.5 8847", ""), point="stock"),
    _scn("five_fixes", BAR, le_script(tp=0.5, **_CYCLE) + "fix loading2 all ex_load 7 1 1 1.12 2 prob 0.4 91823 iparam 1 1 jparam 1 1\n"
         "fix unloading2 all ex_unload 9 2 0.8 prob 0.2 55113\nrun 64\n", fixes=LE3 + ("loading2", "unloading2"), point="five"),
    # anchored beads: type 4 is outside the group that nve, langevin and the LE fixes act on
    _scn("group_anchored", dict(n=N, types=("anchored", 5)), _GROUP + "run 64\n", mid=32, family="group", point="anchored"),
    _scn("langevin_scale_zero", BAR, le_script(tp=0.5, **_CYCLE).replace("1.0 1.0 1.0 904297", "1.0 1.0 1.0 904297 scale 2 1.5 zero yes")
         + "run 64\n", contrast=(" scale 2 1.5 zero yes", ""), family="langevin", mid=32),
    # r-RESPA: ex_load and ex_unload act at the outermost level; fix extrusion never acts (its setmask() has no
    # POST_INTEGRATE_RESPA, oracle/AUDIT.md row R1) - kept as the reference has it, and asserted as such
    _scn("respa2", BAR, le_script(tp=0.5, **_CYCLE) + "run_style respa 2 4\nrun 44\n", steps=44, contrast=("run_style respa 2 4\n", ""),
         idle=("loop",), family="respa", mid=22),
    _scn("respa3", BAR, le_script(tp=0.5, **_CYCLE) + "run_style respa 3 2 2 bond 1 pair 3\nrun 44\n", steps=44,
         contrast=("run_style respa 3 2 2 bond 1 pair 3\n", ""), idle=("loop",)),
    # semiflexible chains; ex_load ... atype 2 makes angles, ex_unload takes them along
    _scn("angle_harmonic", dict(n=N, nchains=2, seed=6, angles=True), ANGLES % ("harmonic", "3.0 170.0", "1.0 100.0") + "run 64\n",
         mid=32, family="angle", point="angles"),
    _scn("angle_cosine", dict(n=N, nchains=2, seed=6, angles=True), ANGLES % ("cosine", "2.5", "0.5") + "run 64\n", point="angles"),
    # a second run command: setup draws another 3N
    _scn("two_runs", BAR, le_script(tp=0.5, **_CYCLE) + "run 32\nrun 32\n", contrast=("run 32\nrun 32\n", "run 64\n")),
    _scn("velocity_loop_all", BAR, le_script(tp=0.5, **_CYCLE) + "velocity all create 1.0 4928 loop all\nrun 32\n"
         "velocity all create 1.2 777 loop all\nrun 32\n", contrast=("create 1.2 777 loop all", "create 1.2 777 loop local")),
    _scn("velocity_loop_local", BAR, le_script(tp=0.5, **_CYCLE) + "velocity all create 1.0 4928 loop local\nrun 32\n"
         "velocity all create 1.2 777 loop local\nrun 32\n", contrast=("create 1.2 777 loop local", "create 1.2 777 loop all")),
    # the barrier cycle and the sorted one for 2 and 3 z slabs
    _scn("slabs_cycle", _SLABS, _DD + "run 60\n", steps=60, contrast=("1 2 3 0.5 2 4", "1 2 3 1.0 2 4"), point="along_z+full_bond"),
    _scn("slabs_sort", _SLABS, _sorted(_DD, 3) + "run 60\n", steps=60, contrast=("atom_modify sort 3 0", "atom_modify sort 0 0"),
         point="along_z+sorted"),
    # fix langevin with a temperature ramp (Tstart 1.0, Tstop 2.0 over the run)
    _scn("langevin_ramp", BAR, le_script(tp=0.5, **_CYCLE).replace("1.0 1.0 1.0 904297", "1.0 2.0 1.0 904297") + "run 64\n",
         contrast=("1.0 2.0 1.0 904297", "1.0 1.0 1.0 904297"), family="langevin"),
]


# ------------------------------------------------------------------------------------------------------------------
# limit scenarios: runs of the reference that END IN AN ERROR because one per-atom row is one slot short, and their twins
# ------------------------------------------------------------------------------------------------------------------
# A limit scenario is a script the reference aborts; its fixture (ref_limit_*.npz) holds the error text, the step, and the
# state after the last complete step.  Its twin is the same script with that one capacity (`extra bond / special / angle per
# atom`) one larger and nothing else changed: an ordinary scenario that runs to the end, whose point is that some bead ends
# with that row exactly full (full_bond, full_special, full_angle) - with every row of every tag compared exactly, a store
# one slot too far shows.  Two twins are scenarios that existed before (slabs_cycle, stock_create).  limit_load_bpa runs the
# slab scenario's script (iparam 1 1): ex_load bonds only beads that hold exactly two bonds, so its maxbond never decides.
def _without(script, *ids):
    return "\n".join(ln for ln in script.split("\n") if not any(ln.startswith("fix %s " % i) for i in ids))


_CYC = le_script(tp=0.5, **_CYCLE)
_LOAD_ONLY = _without(le_script(nl=5, lprob="prob 0.8 684474"), "loop", "unloading")
# one extruder bond across the junction of two chains (beads 250 | 251 of four chains of 250): both of its ends hold two
# bonds, every bead it can step to holds two, and with `extra bond per atom` 0 two is all a row has.  tp = 0: a barrier bead
# of the blocking side never lets the extruder through, so exactly one end tries to step (thermo 1: the one move is printed)
_EXT_ONLY = _without(le_script(n1=4, tp=0.0, lr=""), "loading", "unloading").replace("thermo 10", "thermo 1")
_JUNCTION = dict(n=N, nchains=4, seed=2, ext_bonds=[(250, 251)])
_ANG = dict(n=N, nchains=2, seed=6, angles=True)
_ANG_SCRIPT = ANGLES % ("harmonic", "3.0 170.0", "1.0 100.0")

SCENARIOS += [
    _scn("twin_load_rebuild_special", dict(BAR, extra_special=5), _LOAD_ONLY + "run 48\n", steps=48, fixes=("loading",),
         point="full_special"),
    _scn("twin_load_angles", dict(_ANG, extra_angle=12), _ANG_SCRIPT + "run 28\n", steps=28, point="full_angle"),
    _scn("twin_ext_bpa_low", dict(_JUNCTION, type_at=[(252, 3)], extra_bond=1), _EXT_ONLY + "run 48\n", steps=48, fixes=("loop",),
         point="full_bond", min_ext=1),
    _scn("twin_ext_rebuild_special", dict(BAR, extra_special=12), _CYC + "run 48\n", steps=48, point="full_special"),
]
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]
BY_NAME["stock_create"]["point"] += "+full_bond"


def _limit(name, system, script, steps, at_limit, twin=None, fixes=LE3, runs_on=False, **kw):
    """at_limit: what reached() asks of the last complete step (bond: a bead with num_bond == bond_per_atom; special12: the 1-2
    block alone fills the special row; multi: a bead with two extruder bonds; twin: the row that overflows is rebuilt whole, no
    bead need be full before - the twin, one slot larger, ends full instead).  runs_on: the reference does NOT stop."""
    s = _scn(name, system, script + "run %d\n" % steps, steps=steps, fixes=fixes, **kw)
    s.update(at_limit=at_limit, twin=twin, runs_on=runs_on, limit=True)
    return s


LIMITS = [
    # (the slab system and script of slabs_cycle: the GPU suite also runs this one on two ranks)
    _limit("limit_load_bpa", dict(_SLABS, extra_bond=0), _DD, 48, "bond", twin="slabs_cycle"),
    # special_bonds fene trims the 1-3 and 1-4 blocks (weights 1.0): a bead no fix has touched lists its two 1-2 partners, and
    # with `extra special per atom` 0 that is the whole row.  No twin: with one slot more the insert passes and the rebuild
    # that follows (7 entries) overflows - that run is limit_load_rebuild_special's kind
    _limit("limit_load_special", dict(BAR, extra_special=0), _CYC, 48, "special12"),
    _limit("limit_load_rebuild_special", dict(BAR, extra_special=4), _LOAD_ONLY, 48, "twin", twin="twin_load_rebuild_special",
           fixes=("loading",)),
    _limit("limit_load_angles", dict(_ANG, extra_angle=11), _ANG_SCRIPT, 28, "twin", twin="twin_load_angles"),
    _limit("limit_ext_multi", dict(BAR, ext_bonds=[(10, 12), (10, 14)], extra_bond=0), _CYC, 48, "multi"),
    _limit("limit_ext_bpa_low", dict(_JUNCTION, type_at=[(252, 3)], extra_bond=0), _EXT_ONLY, 48, "bond", twin="twin_ext_bpa_low",
           fixes=("loop",)),
    _limit("limit_ext_bpa_high", dict(_JUNCTION, type_at=[(249, 2)], extra_bond=0), _EXT_ONLY, 48, "bond", fixes=("loop",),
           runs_on=True, point="one_sided", min_ext=1),
    _limit("limit_ext_rebuild_special", dict(BAR, extra_special=11), _CYC, 48, "twin", twin="twin_ext_rebuild_special"),
    _limit("limit_create_bpa", dict(n=N, types=("sticky",), extra_bond=0), STOCK % "", 60, "bond", twin="stock_create",
           fixes=("creating", "breaking")),
    _limit("limit_create_special", dict(n=N, types=("sticky",), extra_special=0), STOCK % "", 60, "special12",
           fixes=("creating", "breaking")),
]
LIMIT_BY_NAME = {s["name"]: s for s in LIMITS}
LIMIT_NAMES = [s["name"] for s in LIMITS]
ERROR_LIMITS = [s["name"] for s in LIMITS if not s["runs_on"]]


def has_angles(scn):
    return bool(scn["system"].get("angles"))


def thermo_columns(scn):
    return ("step",) + THERMO + tuple("f_%s[%d]" % (f, k) for f in scn["fixes"] for k in (1, 2))


def record_lines(scn, prefix, every):
    """What the reference runs on top of the script, in front of its first run command: the thermo columns, the bond and
    angle rows through compute property/local + dump local (every step), the per-atom state every `every` steps in LOCAL
    order (the reader sorts by id and keeps the order)."""
    out = ["thermo_style custom " + " ".join(thermo_columns(scn)), "thermo_modify format float %.15g",
           "compute rrb all property/local btype batom1 batom2",
           "compute rrl all bond/local dist",          # (the same bonds in the same order as property/local)
           "dump rrb all local 1 %s.bonds index c_rrb[1] c_rrb[2] c_rrb[3] c_rrl" % prefix,
           "dump rrs all custom %d %s.state id type x y z ix iy iz vx vy vz fx fy fz" % (every, prefix),
           "dump_modify rrs format float %.17g"]
    if has_angles(scn):
        out += ["compute rra all property/local atype aatom1 aatom2 aatom3",
                "dump rra all local 1 %s.angles index c_rra[1] c_rra[2] c_rra[3] c_rra[4]" % prefix]
    if scn.get("limit"):
        # a run that is meant to abort: every dump and the thermo output flushed after every step, so that the last complete
        # step survives; thermo after every step (the row of the last complete step is the one kept); and the per-atom bond
        # count, which the bond rows cannot give once a bond is stored by one end only
        out += ["compute rrn all property/atom nbonds", "dump rrn all custom %d %s.nbonds id c_rrn" % (every, prefix),
                "thermo 1", "thermo_modify flush yes"]
        out += ["dump_modify %s flush yes" % d for d in ["rrb", "rrs", "rrn"] + (["rra"] if has_angles(scn) else [])]
    return "\n".join(out) + "\n"


def reference_script(scn, prefix, every):
    lines = scn["script"].split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("velocity "))
    first_run = next(i for i, ln in enumerate(lines) if ln.startswith("run "))
    assert all(ln.startswith(("run ", "velocity ", "run_style")) or not ln for ln in lines[k:]) and first_run >= k
    return "\n".join(lines[:k]) + "\n" + record_lines(scn, prefix, every) + "\n".join(lines[k:])


def capacities(system):
    """bond_per_atom, maxspecial and angle_per_atom as read_data sets them for a start system: the largest count in the file
    plus the `extra ... per atom` line.  Every script here says `special_bonds fene`, whose 1-3 and 1-4 weights of 1.0 make
    the special build keep the 1-2 block only (Special::trim): the longest row of the file is the largest bond count."""
    n = len(system["x"])
    nb = np.bincount(np.asarray(system["bonds"])[:, 1:].reshape(-1) - 1, minlength=n).max()
    out = dict(bond=int(nb + system.get("extra_bond", 0)), special=int(nb + system.get("extra_special", 0)), angle=0)
    if system.get("nangletypes"):          # (newton_bond off: an angle of the file is stored at its three atoms)
        out["angle"] = int(np.bincount(np.asarray(system["angles"])[:, 1:].reshape(-1) - 1, minlength=n).max() + system.get("extra_angle", 0))
    return out


def bonds_per_bead(rows, n):
    return np.bincount(np.asarray(rows)[:, 1:].reshape(-1) - 1, minlength=n)


def within_three_bonds(rows, n):
    """Per bead the number of other beads at most three bonds away: the length of a special row that has been rebuilt whole
    (1-2, 1-3 and 1-4 partners, each once)."""
    nbr = [set() for _ in range(n)]
    for _, a, b in np.asarray(rows):
        nbr[a - 1].add(b - 1), nbr[b - 1].add(a - 1)
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        seen, edge = {i}, {i}
        for _ in range(3):
            edge = set().union(*[nbr[j] for j in edge]) - seen if edge else set()
            seen |= edge
        out[i] = len(seen) - 1
    return out


def script_for_steps(scn, steps):
    """The scenario's script cut to `steps` steps: a fresh run that long is the state after step `steps` of the full run."""
    out, left = [], steps
    for ln in scn["script"].split("\n"):
        if ln.startswith("run "):
            if left <= 0:
                break
            k = min(int(ln.split()[1]), left)
            left -= k
            ln = "run %d" % k
        elif ln.startswith("velocity ") and left <= 0:
            break
        out.append(ln)
    assert left == 0, (scn["name"], steps)
    # a temperature ramp runs from Tstart to Tstop over the steps of the run command: the cut run ramps to the temperature the
    # full run has reached at the cut (1.0 -> 2.0 over 64 steps: a multiple of 1/64, exact in binary; the target of a step
    # then differs from the full run's by the rounding of step / steps * (steps / 64) alone)
    total = sum(int(ln.split()[1]) for ln in scn["script"].split("\n") if ln.startswith("run "))
    for k, ln in enumerate(out):
        w = ln.split()
        if w[:1] == ["fix"] and w[3] == "langevin" and w[4] != w[5] and steps != total:
            assert scn["script"].count("\nrun ") == 1 and steps > 0
            w[5] = repr(float(w[4]) + (float(w[5]) - float(w[4])) * steps / total)
            out[k] = " ".join(w)
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------------------------
class Fixture:
    """One recorded run.  rows_at(step) / angles_at(step): the multiset (sorted array) after that step."""

    def __init__(self, name):
        import json
        limit = name in LIMIT_BY_NAME
        self.name, self.scn = name, (LIMIT_BY_NAME if limit else BY_NAME)[name]
        with np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)) as z:
            self.z = {k: z[k] for k in z.files}
        with open(os.path.join(GOLDEN, "ref_runs.json")) as fh:
            self.meta = json.load(fh)["limits" if limit else "scenarios"][name]
        # (a limit fixture: one checkpoint, the last complete step; the error came in the step after it)
        self.error, self.error_step = self.meta.get("error"), self.meta.get("error_step")
        self.checkpoints = [int(c) for c in self.z["checkpoints"]]
        self.last = self.checkpoints[-1]
        self.columns = thermo_columns(self.scn)

    def system(self):
        return build_system(self.scn, recorded=self.z)

    def _at(self, what, step):
        steps = self.z[what + "_steps"]
        k = int(np.searchsorted(steps, step, side="right")) - 1
        lo, hi = self.z[what + "_offsets"][k], self.z[what + "_offsets"][k + 1]
        return self.z[what + "_rows"][lo:hi]

    def rows_at(self, step):
        return self._at("bond", step)

    def angles_at(self, step):
        return self._at("angle", step)

    def change_steps(self, what="bond"):
        return [int(s) for s in self.z[what + "_steps"]]

    def state(self, step):
        k = self.checkpoints.index(step)
        if "x" not in self.z:          # a run that ended in its first step: its last complete state is the start it read, which
            s = self.system()          # the generator has compared with the reference's own step-0 dump bit for bit
            return dict(x=np.asarray(s["x"]), v=np.asarray(s["v"]), type=np.asarray(s["type"]), image=np.asarray(s["image"]))
        return {q: self.z[q][k] for q in ("x", "v", "type", "image")}

    def unwrapped(self, x, image):
        box = np.asarray(self.system_box())
        return np.asarray(x) + np.asarray(image) * (box[:, 1] - box[:, 0])[None, :]

    def system_box(self):
        return lattice_start(self.scn["system"]["n"], self.scn["system"].get("nchains", 1), self.scn["system"].get("seed", 1))["box"]

    def thermo(self):
        return self.z["thermo"]

    def col(self, name):
        return self.columns.index(name)

    def spread(self, what, step=None):
        m = self.meta["spread"]
        return float(m[what][str(step)]) if step is not None else m[what]


def bond_rows(nb, bt, ba):
    """Per-atom bond tables (newton_bond off: every bond stored at both ends) -> sorted (type, lower id, higher id) rows, one
    per bond, duplicates kept."""
    nb, bt, ba = np.asarray(nb), np.asarray(bt), np.asarray(ba)
    if bt.ndim == 1:
        bt, ba = bt.reshape(-1, 1), ba.reshape(-1, 1)
    i, m = np.nonzero(np.arange(bt.shape[1])[None, :] < nb[:, None])
    own, other = i + 1, ba[i, m]
    keep = own < other
    rows = np.stack([bt[i, m][keep], own[keep], other[keep]], axis=1).astype(np.int64)
    return sort_rows(rows)


def angle_rows(na, at, a1, a2, a3):
    """Per-atom angle tables -> the copies the centre atoms store, as sorted (type, a1, a2, a3) rows with a1, a3 as stored,
    duplicates kept: what compute property/local lists with newton_bond off."""
    na, at, a1, a2, a3 = (np.asarray(q) for q in (na, at, a1, a2, a3))
    if at.ndim == 1:
        at, a1, a2, a3 = (q.reshape(-1, 1) for q in (at, a1, a2, a3))
    i, m = np.nonzero(np.arange(at.shape[1])[None, :] < na[:, None])
    keep = a2[i, m] == i + 1
    rows = np.stack([at[i, m][keep], a1[i, m][keep], a2[i, m][keep], a3[i, m][keep]], axis=1).astype(np.int64)
    return sort_rows(rows)


def sort_rows(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, rows.shape[1] if rows.ndim == 2 else 3)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def pressure_tensor(box, mass_per_atom, v, virial6, n):
    """pxx pyy pzz pxy pxz pyz of compute pressure in lj units from velocities and the summed virial (xx yy zz xy xz yz)."""
    box = np.asarray(box)
    vol = float(np.prod(box[:, 1] - box[:, 0]))
    v = np.asarray(v, dtype=np.longdouble)
    m = np.asarray(mass_per_atom, dtype=np.longdouble)
    ke = [float((m * v[:, a] * v[:, b]).sum()) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    return np.array([(ke[k] + virial6[k]) / vol for k in range(6)])


# ------------------------------------------------------------------------------------------------------------------
# the comparison (CPU: the oracle; GPU: the engine - the same code)
# ------------------------------------------------------------------------------------------------------------------
# A thermo value is recorded at 15 significant digits: up to 5e-15 of its size is lost in the record alone, whatever the
# spread says (temp at step 0 has a spread of exactly 0: the perturbed starts share their velocities).
THERMO_FLOOR = 5e-15


def thermo_bound(fx, row, name, oracle_dev=0.0):
    sp = np.asarray(fx.spread("thermo"))[row, fx.col(name) - 1]
    val = abs(fx.thermo()[row, fx.col(name)])
    return FACTOR * max(sp, THERMO_FLOOR * max(val, 1.0), oracle_dev)


def check_discrete(fx, step, got):
    """got: dict with bond (rows), angle (rows or None), type, image, and - at thermo steps - bonds, angles, fixvec {id: (a, b)}."""
    bad = []
    ref = fx.rows_at(step)
    if not np.array_equal(got["bond"], ref):
        bad.append("step %d: bond rows differ (%d against %d recorded)" % (step, len(got["bond"]), len(ref)))
    if has_angles(fx.scn):
        ra = fx.angles_at(step)
        if not np.array_equal(got["angle"], ra):
            bad.append("step %d: angle rows differ (%d against %d recorded)" % (step, len(got["angle"]), len(ra)))
    if step in fx.checkpoints:
        st = fx.state(step)
        if not np.array_equal(got["type"], st["type"]):
            bad.append("step %d: types differ on %d beads" % (step, (got["type"] != st["type"]).sum()))
        if not np.array_equal(got["image"], st["image"]):
            bad.append("step %d: image flags differ on %d beads" % (step, (got["image"] != st["image"]).any(axis=1).sum()))
    th = fx.thermo()
    k = np.nonzero(th[:, 0] == step)[0]          # (of a step printed twice, the last row: the state the run went on from)
    if len(k) and "bonds" in got:
        row = th[k[-1]]
        if got["bonds"] != row[fx.col("bonds")]:
            bad.append("step %d: bonds %r against %r" % (step, got["bonds"], row[fx.col("bonds")]))
        if got.get("angles") is not None and got["angles"] != row[fx.col("angles")]:
            bad.append("step %d: angles %r against %r" % (step, got["angles"], row[fx.col("angles")]))
        for fid, (a, b) in got.get("fixvec", {}).items():
            want = (row[fx.col("f_%s[1]" % fid)], row[fx.col("f_%s[2]" % fid)])
            if (a, b) != want:
                bad.append("step %d: fix %s vector %r against %r" % (step, fid, (a, b), want))
    return bad


def deviation(fx, step, x, image, v, f=None):
    """Largest |dx| (unwrapped), |dv| and |df| against the recorded state."""
    st = fx.state(step)
    out = dict(x=float(np.abs(fx.unwrapped(x, image) - fx.unwrapped(st["x"], st["image"])).max()),
               v=float(np.abs(np.asarray(v) - st["v"]).max()))
    if f is not None:
        out["f"] = float(np.abs(np.asarray(f) - fx.z["f"]).max())
    return out


def check_continuous(fx, step, dev, label, oracle_dev=None):
    """dev under FACTOR x max(recorded spread, oracle_dev): oracle_dev is the oracle's own deviation from the same fixture (the
    GPU tests pass it; the oracle itself is held to the spread alone)."""
    bad = []
    for q, err in dev.items():
        sp = fx.spread(q, step)
        b = FACTOR * max(sp, (oracle_dev or {}).get(q, 0.0))
        print("%-34s %s after step %3d: %.2e  spread %.2e  oracle %.2e  bound %.2e" %
              (label, q, step, err, sp, (oracle_dev or {}).get(q, float("nan")), b))
        if not err <= b:
            bad.append("%s %s after step %d: %.3e exceeds %.3e" % (label, q, step, err, b))
    return bad


def thermo_deviation(fx, rows, names):
    """rows: the thermo rows of a run of fx.last steps, in order, as dicts with `step` -> {(row index, name): |difference|}
    against the recorded rows; the k-th row is the k-th recorded one (a step can print twice: two runs)."""
    th, out = fx.thermo(), {}
    assert [r["step"] for r in rows] == [int(s) for s in th[:, 0]], ([r["step"] for r in rows], th[:, 0])
    for k, got in enumerate(rows):
        for nm in names:
            if nm in got:
                out[(k, nm)] = abs(got[nm] - th[k, fx.col(nm)])
    return out


def check_thermo(fx, dev, label, oracle_dev=None):
    bad, worst = [], {}
    for (k, nm), err in dev.items():
        b = thermo_bound(fx, k, nm, (oracle_dev or {}).get((k, nm), 0.0))
        rel = err / b
        if rel > worst.get(nm, (-1.0,))[0]:
            worst[nm] = (rel, err, b, k)
        if not err <= b:
            bad.append("%s thermo %s row %d: %.3e exceeds %.3e" % (label, nm, k, err, b))
    for nm, (rel, err, b, k) in sorted(worst.items()):
        print("%-34s thermo %-7s worst at row %2d: %.2e  bound %.2e" % (label, nm, k, err, b))
    return bad


# ------------------------------------------------------------------------------------------------------------------
# the oracle side (shared: the CPU tests assert on it, the GPU tests take their second bound from it)
# ------------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def oracle_run(name, steps=None):
    """The oracle after `steps` steps of the scenario (default: all), as the dict check_discrete takes plus x, v, f, rows."""
    from systems import run_oracle
    fx = fixture(name)
    steps = fx.last if steps is None else steps
    if (name, steps) in _oracle_cache:
        return _oracle_cache[(name, steps)]
    s = fx.system()
    o = run_oracle(script_for_steps(fx.scn, steps), s)
    nb, bt, ba = o.bond_table()
    got = dict(bond=bond_rows(nb, bt, ba), angle=None, type=o.types().copy(), image=o.image().copy(), x=o.x(), v=o.v(), f=o.f(),
               bonds=float(o.nbonds()), fixvec={fid: tuple(float(q) for q in o.fix_vector(fid)) for fid in fx.scn["fixes"]},
               builds=int(o.neigh_builds()), local_order=o.local_order().copy())
    if has_angles(fx.scn):
        got["angle"] = angle_rows(*o.angle_table())
        got["angles"] = float(o.nangles())
    hist = o.thermo_history()
    got["rows"] = [dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5], bonds=r[15]) for r in hist]
    t = o.thermo()
    mass = np.asarray(s["mass"])[got["type"] - 1]
    p6 = pressure_tensor(s["box"], mass, got["v"], t[8:14], len(mass))
    got["rows"][-1].update(dict(zip(("pxx", "pyy", "pzz", "pxy", "pxz", "pyz"), p6)))
    _oracle_cache[(name, steps)] = got
    return got


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def reached(fx):
    """The scenario's own point, told from the recorded run (condition (d); the contrast runs are the generator's and their
    outcome is in ref_runs.json)."""
    if fx.scn["contrast"] and not fx.meta["contrast_differs"]:
        return False
    return all(_reached(fx, point) for point in fx.scn["point"].split("+"))


def _reached(fx, point):
    scn, last = fx.scn, fx.last
    rows = fx.rows_at(last)
    ext = rows[rows[:, 0] == 2]
    if point == "stall":          # an extruder bond that two consecutive extrusion firings left where it was, and a wide loop
        before = fx.rows_at(last - 11)          # n1 = 5: two extrusion firings earlier
        held = len(set(map(tuple, before[before[:, 0] == 2])) & set(map(tuple, ext))) > 0
        return bool(held and (ext[:, 2] - ext[:, 1]).max() >= 6)
    if point == "chains":
        per = scn["system"]["n"] // scn["system"]["nchains"]
        return len(set((ext[:, 1] - 1) // per)) >= 2 and bool(((ext[:, 1] - 1) // per == (ext[:, 2] - 1) // per).all())
    if point == "straddle":
        st = fx.state(last)
        box = np.asarray(fx.system_box())
        d = np.abs(st["x"][ext[:, 1] - 1] - st["x"][ext[:, 2] - 1])
        return bool((d > 0.5 * (box[:, 1] - box[:, 0])[None, :]).any())
    if point == "along_z":        # at the end at least two extruder bonds across a face between 2 slabs and between 3 slabs,
        st, box = fx.state(last), np.asarray(fx.system_box())          # and none longer than 3.0 after any step
        z = (st["x"][:, 2] - box[2, 0]) / (box[2, 1] - box[2, 0])
        across = all(((z[ext[:, 1] - 1] * w).astype(int) != (z[ext[:, 2] - 1] * w).astype(int)).sum() >= 2 for w in (2, 3))
        return bool(across and fx.meta["longest_extruder_bond"] < 3.0)
    if point == "sorted":
        return bool((fx.z["local_order"] != np.arange(1, len(fx.z["local_order"]) + 1)).any())
    if point == "file_order":
        return bool(np.array_equal(fx.z["local_order"], fx.system()["file_order"] + 1))
    if point == "stock":
        th = fx.thermo()[-1]
        return th[fx.col("f_creating[2]")] > 10 and th[fx.col("f_breaking[2]")] > 0
    if point == "five":
        th = fx.thermo()[-1]
        return th[fx.col("f_loading2[2]")] > 0 and th[fx.col("f_unloading2[2]")] > 0
    if point == "anchored":
        s = fx.system()
        anchor = s["type"] == 4
        st = fx.state(last)
        return bool(anchor.sum() > 20 and np.array_equal(st["x"][anchor], s["x"][anchor]) and not np.array_equal(st["x"][~anchor], s["x"][~anchor]))
    if point == "angles":         # type-2 angles exist, some were taken along by ex_unload
        counts = fx.thermo()[:, fx.col("angles")]
        a = fx.angles_at(last)
        steps = fx.change_steps("angle")
        shrank = any(len(fx.angles_at(steps[k + 1])) < len(fx.angles_at(steps[k])) for k in range(len(steps) - 1))
        return bool((a[:, 0] == 2).any() and shrank and counts.max() > counts[0])
    n, cap = scn["system"]["n"], capacities(fx.system())
    if point == "full_bond":      # a twin: some bead ends with its bond row exactly full
        return bool(bonds_per_bead(rows, n).max() == cap["bond"])
    if point == "full_special":   # some bead ends with a rebuilt special row exactly as long as the row is
        return bool(within_three_bonds(rows, n).max() == cap["special"])
    if point == "full_angle":     # the reference writes no per-atom angle count (and ex_load does not store a new angle at all
        return full_angle(fx)     # three atoms, so the rows do not give it): see full_angle
    if point == "one_sided":      # a bond that one end alone stores: the rows count more bonds on a bead than it holds
        return bool((bonds_per_bead(rows, n) != fx.z["num_bond"]).sum() == 1)
    return True


def full_angle(fx):
    """The twin of the angle limit ends with an angle row exactly full.  The count comes from the oracle at the end of the
    recorded run (its angle rows, the centre copies, are the recorded ones there: check_discrete), bounded from below by the
    recorded rows: centre copies + the end copies ex_load makes."""
    from systems import run_oracle
    o = run_oracle(fx.scn["script"], fx.system())
    table = o.angle_table()
    return bool(np.array_equal(angle_rows(*table), fx.angles_at(fx.last)) and table[0].max() == capacities(fx.system())["angle"])


def at_limit(fx):
    """A limit fixture: the bead the error names sits at its limit after the last complete step (LIMITS: at_limit)."""
    kind, n, cap = fx.scn["at_limit"], fx.scn["system"]["n"], capacities(fx.system())
    rows = fx.rows_at(fx.last)
    if kind == "bond" and fx.scn["runs_on"]:          # (the bead that could not store its end of the new bond is still full)
        short = np.nonzero(bonds_per_bead(rows, n) != fx.z["num_bond"])[0]
        return bool(len(short) == 1 and fx.z["num_bond"][short[0]] == cap["bond"])
    if kind == "bond":
        return bool(bonds_per_bead(rows, n).max() == cap["bond"] and np.array_equal(bonds_per_bead(rows, n), fx.z["num_bond"]))
    if kind == "special12":       # no fix has acted yet (the rows are the file's), so every row is its 1-2 block alone
        return bool(np.array_equal(rows, sort_rows(np.asarray(fx.system()["bonds"]))) and bonds_per_bead(rows, n).max() == cap["special"])
    if kind == "multi":
        ext = rows[rows[:, 0] == 2]
        return bool(np.bincount(ext[:, 1:].reshape(-1)).max() == 2)
    if kind == "twin":            # a row rebuilt whole overflows from any length below: the twin, one slot longer, ends full
        return bool(reached(fixture(fx.scn["twin"])))
    return False


def limit_conditions(fx):
    """What the generator asks of a limit scenario before it writes it, and the tests of the committed file: one kind of
    ERROR, at one step, in all four runs; the bead at its limit; the twin there, the same script with one slot more."""
    scn = fx.scn
    if scn["runs_on"]:
        return fixture_conditions(fx) or ("" if at_limit(fx) else "the full bead is not full")
    m = fx.meta
    if not (m["error_kinds"] == 1 and m["perturbed_reruns"] == 3 and m["perturbed_same_error"] is True and m["perturbed_rows_identical"] is True):
        return "the reruns do not end in the one error"
    if m["error_step"] != fx.last + 1 or not 1 <= m["error_step"] <= scn["checkpoints"][-1]:
        return "the error step is not the step after the last complete one"
    if not at_limit(fx):
        return "no bead at its limit after the last complete step"
    if scn["twin"]:
        tw = BY_NAME[scn["twin"]]
        a, b = dict(scn["system"]), dict(tw["system"])
        key = [k for k in ("extra_bond", "extra_special", "extra_angle") if a.get(k) != b.get(k)]
        default = dict(extra_bond=1, extra_special=20, extra_angle=24)
        if len(key) != 1 or b.get(key[0], default[key[0]]) != a[key[0]] + 1:
            return "the twin is not one slot larger"
        a.pop(key[0]), b.pop(key[0], None)
        if a != b or script_for_steps(tw, 1) != script_for_steps(scn, 1):
            return "the twin differs in more than the capacity"
        if not any(p.startswith("full_") for p in tw["point"].split("+")):
            return "the twin has no full row as its point"
    return ""


def fixture_conditions(fx):
    """(c) and (d) from a fixture; '' when they hold (the generator refuses a run that fails them, test_reference_runs_cpu.py asks the same of the committed files)."""
    th = fx.thermo()
    for fid in fx.scn["fixes"]:          # (fix extrusion reports its moves in the first entry only)
        acted = max(th[:, fx.col("f_%s[1]" % fid)].max(), th[:, fx.col("f_%s[2]" % fid)].max()) > 0
        if acted == (fid in fx.scn["idle"]):
            return "(c) fix %s %s" % (fid, "acted" if acted else "never acted")
    rows = fx.rows_at(fx.last)
    if (rows[:, 0] == 2).sum() < fx.scn["min_ext"]:
        return "(c) %d type-2 bonds at the end" % (rows[:, 0] == 2).sum()
    if not reached(fx):
        return "(d) the scenario's point was not reached"
    return ""
