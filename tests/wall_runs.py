"""The scenarios of the recorded reference runs with fix wall/region (tests/golden/wall_*.npz, wall_runs.json) and what the
tests need to read them.  tests/golden/make_wall_runs.py runs the reference binary on each and stores numbers only;
test_wall_cpu.py holds wall_reference.py and the conditions on the fixtures to them, test_gpu_wall.py the HIP path.

(a) `run 0` on a compressed chain - 343 beads on the jittered lattice of systems.lattice_chain, one lattice spacing apart - for
    the five styles and each region of REGIONS: forces with and without the wall, f_ID, f_ID[1..3], pe and press with
    fix_modify energy / virial no and yes.  The regions are placed so that every surface has beads within the cutoff:
    every face of the block, the curved surface and both caps of the cylinder, faces, edges and a corner of the block seen
    from outside.
(b) the LE cycle of reference_runs.py (cycle_tp05) inside a WCA sphere (lj126, cutoff 2^(1/6)), from a start the reference
    itself prepared: the melt of reference_runs, unwrapped, in a box widened by 8 sigma per side, pressed into the sphere by harmonic walls
    of shrinking radius and then left to settle against the WCA wall (wall_melt.npz; compared with nothing).
(c) two runs on one handle with the wall unfixed in between.
"""
import json
import os

import numpy as np

import reference_runs as rr
from systems import CHAIN_SCRIPT, lattice_chain, le_script

GOLDEN = rr.GOLDEN
STYLES = {
    "lj93": "lj93 1.0 1.0 1.2",
    "lj126": "lj126 1.0 1.0 1.1",
    "lj1043": "lj1043 1.0 1.0 1.25",
    "harmonic": "harmonic 7.5 0.0 1.0",
    "morse": "morse 1.5 2.0 0.6 1.15",
}
A_N, A_SEED = 343, 11


def a_system():
    return lattice_chain(A_N, seed=A_SEED)


def _a_regions():
    s = a_system()
    L = float(s["box"][0][1])
    c = 0.5 * L
    return {
        # every bead inside, the corner beads of the lattice within the cutoff
        "sphere_in": "sphere %.17g %.17g %.17g 6.05 side in" % (c, c, c),
        # a ball beside the lattice, centre outside the box: the beads of one face within the cutoff of it
        "sphere_out": "sphere -1.2 %.17g %.17g 1.2 side out" % (c, c),
        # the six faces just inside the box faces: the outer layer of the lattice within the cutoff, corner beads of three faces
        "block_in": "block 0.02 %.17g 0.05 %.17g 0.08 %.17g side in" % (L - 0.02, L - 0.05, L - 0.08),
        # a slab beside the lattice: beads opposite its face, beside its edges and off its corners
        "block_out": "block -3.0 0.0 2.0 5.0 2.5 %.17g side out" % (L + 2.0),
        "cylinder_in": "cylinder z %.17g %.17g 5.0 0.02 %.17g side in" % (c, c, L - 0.05),
        # (beyond the five of the issue: the two other axes)
        "cylinder_x_in": "cylinder x %.17g %.17g 5.0 0.05 %.17g side in" % (c, c, L - 0.02),
        "cylinder_y_in": "cylinder y %.17g %.17g 5.0 0.08 %.17g side in" % (c, c, L - 0.05),
    }


REGIONS = _a_regions()
A_THERMO = ("step", "pe", "press", "f_w", "f_w[1]", "f_w[2]", "f_w[3]")


def a_script(region, style, wall=True):
    """What the engine runs for one (a) case: the first `run 0` with fix_modify at its defaults (no, no), the second with both on."""
    s = CHAIN_SCRIPT + "fix 1 all nve\n"
    if not wall:
        return s + "thermo_style custom step pe press\nrun 0\n"
    return s + ("region R %s\nfix w all wall/region R %s\nthermo_style custom %s\nrun 0\nfix_modify w energy yes virial yes\nrun 0\n"
                % (REGIONS[region], STYLES[style], " ".join(A_THERMO)))


def a_fixture(region):
    """-> dict: f0 (no wall), pe0, press0, and per style f, rows (2, 7): the thermo rows of the two `run 0`."""
    with np.load(os.path.join(GOLDEN, "wall_a_%s.npz" % region)) as z:
        return {k: z[k] for k in z.files}


def meta():
    with open(os.path.join(GOLDEN, "wall_runs.json")) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------------------------
# (b), (c): the LE cycle inside a WCA sphere
# ------------------------------------------------------------------------------------------------------------------
B_N, B_SEED, B_PAD = 1000, 1, 8.0
B_RADIUS = 7.0
B_CUT = 1.122462048309373          # 2^(1/6)
B_STEPS = 48
B_SHRINK = 0.3                    # the preparation's harmonic sphere shrinks by this much every 300 steps


def b_box():
    box = np.asarray(rr.lattice_start(B_N, 1, B_SEED)["box"], dtype=np.float64)
    return np.stack([box[:, 0] - B_PAD, box[:, 1] + B_PAD], axis=1)


def b_centre():
    return b_box().mean(axis=1)


def b_region(radius=B_RADIUS, name="ball"):
    c = b_centre()
    return "region %s sphere %.17g %.17g %.17g %.17g side in\n" % (name, c[0], c[1], c[2], radius)


def b_melt_script(farthest):
    """The preparation the reference runs (generator only): harmonic walls of shrinking radius from beyond the farthest bead
    down to B_RADIUS, then the WCA wall."""
    radii = [B_RADIUS + B_SHRINK * k for k in range(int(np.ceil((farthest + 0.6 - B_RADIUS) / B_SHRINK)), -1, -1)]
    s = CHAIN_SCRIPT + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 4242\n"
    for k, r in enumerate(radii):
        s += b_region(r, "s%d" % k) + "fix w all wall/region s%d harmonic 10.0 0.0 1.5\nrun 300\nunfix w\n" % k
    s += "fix w all wall/region s%d harmonic 50.0 0.0 1.2\nrun 300\nunfix w\n" % (len(radii) - 1)
    s += "fix w all wall/region s%d lj126 1.0 1.0 %.17g\nrun 600\n" % (len(radii) - 1, B_CUT)
    return s


def b_system(recorded=None):
    """The start of the (b) / (c) scenarios: the prepared globule (wall_melt.npz) in the widened box, barrier types of cycle_tp05."""
    s = rr.lattice_start(B_N, 1, B_SEED)
    s["box"] = b_box()
    with np.load(os.path.join(GOLDEN, "wall_melt.npz")) as z:
        s["x"], s["v"], s["image"] = z["x"].copy(), z["v"].copy(), z["image"].copy()
    s["type"] = recorded["start_type"].copy() if recorded is not None else rr.barrier_types(B_N, 5, 0.3)
    return s


_LE = le_script(tp=0.5, n1=4, nl=5, nu=6)
_WALL = b_region() + "fix w all wall/region ball lj126 1.0 1.0 %.17g\n" % B_CUT
_WALL_E = _WALL + "fix_modify w energy yes virial yes\n"


def _before_langevin(script, wall):
    return script.replace("fix 2 all langevin", wall + "fix 2 all langevin")


def _scn(name, script, wall_columns=True, fixes=rr.LE3, idle=(), point=""):
    return dict(name=name, system=dict(n=B_N), script=script, checkpoints=[B_STEPS], fixes=fixes, idle=idle, point=point,
                wall_columns=wall_columns, family=None, contrast=None, min_ext=3)


SCENARIOS = [
    _scn("langevin_then_wall", _LE + _WALL_E + "run %d\n" % B_STEPS),
    _scn("wall_then_langevin", _before_langevin(_LE, _WALL_E) + "run %d\n" % B_STEPS),
    _scn("sort3", _LE.replace("atom_modify sort 0 0", "atom_modify sort 3 0") + _WALL_E + "run %d\n" % B_STEPS, point="sorted"),
    _scn("respa2", _LE + _WALL_E + "run_style respa 2 4\nrun %d\n" % B_STEPS, idle=("loop",)),
    _scn("group", _LE + "group low type 1 2\n" + _WALL_E.replace("fix w all", "fix w low") + "run %d\n" % B_STEPS),
    _scn("unfix_between", _LE + _WALL + "run %d\nunfix w\nrun %d\n" % (B_STEPS // 2, B_STEPS // 2), wall_columns=False),
]
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]
WALL_COLUMNS = ("pe", "f_w", "f_w[1]", "f_w[2]", "f_w[3]")


def thermo_columns(scn):
    return rr.thermo_columns(scn) + (WALL_COLUMNS if scn["wall_columns"] else ())


def record_lines(scn, prefix, every):
    """rr.record_lines with the wall's columns behind the others."""
    return rr.record_lines(scn, prefix, every).replace("thermo_style custom " + " ".join(rr.thermo_columns(scn)),
                                                       "thermo_style custom " + " ".join(thermo_columns(scn)))


def reference_script(scn, prefix, every):
    lines = scn["script"].split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("run_style"))
    return "\n".join(lines[:k]) + "\n" + record_lines(scn, prefix, every) + "\n".join(lines[k:])


class Fixture(rr.Fixture):
    def __init__(self, name):
        self.name, self.scn = name, BY_NAME[name]
        with np.load(os.path.join(GOLDEN, "wall_b_%s.npz" % name)) as z:
            self.z = {k: z[k] for k in z.files}
        self.meta = meta()["scenarios"][name]
        self.checkpoints = [int(c) for c in self.z["checkpoints"]]
        self.last = self.checkpoints[-1]
        self.columns = thermo_columns(self.scn)

    def system(self):
        return b_system(recorded=self.z)

    def system_box(self):
        return b_box()


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def near_wall_fraction(x, member=None):
    """Fraction of the beads (of the wall's group) within the cutoff of the (b) sphere, and whether any is outside it."""
    d = np.sqrt(((np.asarray(x) - b_centre()[None, :]) ** 2).sum(axis=1))
    if member is not None:
        d = d[member]
    return float((d > B_RADIUS - B_CUT).mean()), bool((d >= B_RADIUS).any())


def group_low(types):
    return (np.asarray(types) == 1) | (np.asarray(types) == 2)


def fixture_conditions(fx):
    """'' when the scenario's fixture holds what it is for: the LE fixes acted (or were idle), extruder bonds exist, at least
    5 % of the beads the wall acts on are within its cutoff at a recorded step, none outside, and the scenario's own point."""
    th = fx.thermo()
    for fid in fx.scn["fixes"]:
        acted = max(th[:, fx.col("f_%s[1]" % fid)].max(), th[:, fx.col("f_%s[2]" % fid)].max()) > 0
        if acted == (fid in fx.scn["idle"]):
            return "fix %s %s" % (fid, "acted" if acted else "never acted")
    rows = fx.rows_at(fx.last)
    if (rows[:, 0] == 2).sum() < fx.scn["min_ext"]:
        return "%d type-2 bonds at the end" % (rows[:, 0] == 2).sum()
    member = group_low(fx.z["type"][-1]) if fx.name == "group" else None
    frac = near_wall_fraction(fx.z["x"][-1], member)[0]
    if fx.name != "unfix_between" and frac < 0.05:
        return "only %.3f of the beads within the wall's cutoff" % frac
    if fx.name != "unfix_between" and near_wall_fraction(fx.z["x"][-1], member)[1]:
        return "a bead outside the sphere"
    if fx.scn["wall_columns"] and not (np.abs(th[:, fx.col("f_w")]).max() > 0):
        return "the wall's energy is zero in every row"
    if fx.scn["point"] == "sorted" and not (fx.z["local_order"] != np.arange(1, len(fx.z["local_order"]) + 1)).any():
        return "Atom::sort left the order alone"
    return ""
