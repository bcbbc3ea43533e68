"""The scenarios of the recorded reference runs with fix spring/self, fix addforce and fix setforce (tests/golden/extforce_*.npz,
extforce_runs.json) and what the tests need to read them.  tests/golden/make_extforce_runs.py runs the reference binary on each
and stores numbers only; test_extforce_cpu.py holds extforce_reference.py and the conditions on the fixtures to them,
test_gpu_extforce.py the HIP path.

(a) `run 0` on a chain of 400 beads on the jittered lattice of systems.lattice_chain: two tethers (xyz and xy, other K) on
    overlapping groups, an addforce with fix_modify energy yes virial yes, a setforce 0 NULL 0 on a group that overlaps the
    tethered ones.  The data file gives the members image flags of +-1 and +-2; every member of a tether is moved by `set atom`
    between the fix command and the run, so that no spring has zero length.  Then the four fixes are removed and `run 0` again:
    the forces the fixes found.
(b) 48 steps of the LE cycle of reference_runs.py (cycle_tp05) on the 2048-bead melt, with the fixes at several places among the
    post-force fixes, one run with a tether defined between two runs, one under r-RESPA, and one in which a pulled, tethered bead
    crosses a periodic face and is wrapped by a later rebuild.
"""
import json
import os

import numpy as np

import extforce_reference as er
import reference_runs as rr
from systems import CHAIN_SCRIPT, lattice_chain, le_script

GOLDEN = rr.GOLDEN

# ------------------------------------------------------------------------------------------------------------------
# (a)
# ------------------------------------------------------------------------------------------------------------------
A_N, A_SEED = 400, 13
A_K, A_K2 = 10.0, 3.5
A_ADD = (0.7, -1.3, 2.1)
A_TETHER = list(range(5, 400, 10))                    # 40 members
A_TETHER2 = list(range(15, 400, 30)) + [7, 8, 9]      # overlaps A_TETHER at 15, 45, ...
A_PULL = list(range(3, 400, 25)) + [5, 15]            # overlaps both tethers
A_PIN = list(range(25, 400, 40)) + [3, 7]             # overlaps the first tether at 25, 65, ..., the pull at 3, the second at 7
A_IMAGES = ((1, 0, 0), (0, -1, 0), (0, 0, 2), (-2, 1, 0), (0, 2, -1), (1, -1, 1), (0, 0, 0), (-1, 0, -2))
A_THERMO = ("step", "pe", "press", "f_s", "f_s2", "f_a", "f_a[1]", "f_a[2]", "f_a[3]", "f_z[1]", "f_z[2]", "f_z[3]")
A_THERMO0 = ("step", "pe", "press")


def a_members():
    return dict(s=er.members(A_N, A_TETHER), s2=er.members(A_N, A_TETHER2), a=er.members(A_N, A_PULL), z=er.members(A_N, A_PIN))


def a_system():
    s = lattice_chain(A_N, seed=A_SEED)
    m = a_members()
    every = np.nonzero(m["s"] | m["s2"] | m["a"] | m["z"])[0]
    for k, i in enumerate(every):
        s["image"][i] = A_IMAGES[k % len(A_IMAGES)]
    return s


def a_moves():
    """(atom id, new x, y, z) of every tethered bead: 0.04 .. 0.12 off its place in the data file, inside the box."""
    s, m = a_system(), a_members()
    rng = np.random.RandomState(A_SEED + 1)
    out = []
    for i in np.nonzero(m["s"] | m["s2"])[0]:
        d = rng.uniform(0.04, 0.12, size=3) * np.where(rng.rand(3) < 0.5, -1.0, 1.0)
        out.append((int(i) + 1,) + tuple(float(v) for v in s["x"][i] + d))
    return out


def a_positions():
    x = a_system()["x"].copy()
    for row in a_moves():
        x[row[0] - 1] = row[1:]
    return x


def a_script():
    """The first `run 0` with the four fixes, the second without them."""
    ids = lambda v: " ".join(str(i) for i in v)      # noqa: E731
    s = CHAIN_SCRIPT + "fix 1 all nve\n"
    s += "group tether id %s\ngroup tether2 id %s\ngroup pull id %s\ngroup pin id %s\n" % (ids(A_TETHER), ids(A_TETHER2), ids(A_PULL), ids(A_PIN))
    s += "fix s tether spring/self %.17g\nfix s2 tether2 spring/self %.17g xy\n" % (A_K, A_K2)
    for row in a_moves():
        s += "set atom %d x %.17g y %.17g z %.17g\n" % row
    s += "fix a pull addforce %.17g %.17g %.17g\nfix_modify a energy yes virial yes\nfix_modify s energy yes\n" % A_ADD
    s += "fix z pin setforce 0 NULL 0\n"
    s += "thermo_style custom %s\nrun 0\n" % " ".join(A_THERMO)
    s += "unfix s\nunfix s2\nunfix a\nunfix z\nthermo_style custom %s\nrun 0\n" % " ".join(A_THERMO0)
    return s


def a_fixes(system):
    """The four fixes for extforce_reference.apply, in the script's order."""
    m = a_members()
    origin = er.unwrapped(system["x"], system["image"], system["box"])
    return [er.spring(A_K, m["s"], origin, "xyz"), er.spring(A_K2, m["s2"], origin, "xy"), er.add(A_ADD, m["a"]),
            er.setforce((0.0, None, 0.0), m["z"])]


def a_reference(f0, n=A_N):
    """extforce_reference on the (a) state from the forces the fixes found -> (f, the thermo row's fix columns in A_THERMO's
    order from f_s on - per atom, as thermo prints extensive values under norm yes -, the fixes' share of pe, of press)."""
    s = a_system()
    f, out = er.apply(a_fixes(s), a_positions(), s["image"], s["box"], f0)
    cols = [out[0]["energy"], out[1]["energy"], out[2]["energy"]] + list(out[2]["foriginal"]) + list(out[3]["foriginal"])
    box = np.asarray(s["box"], dtype=np.longdouble)
    vol = np.prod(box[:, 1] - box[:, 0])
    pe = (out[0]["energy"] + out[2]["energy"]) / n                 # fix_modify energy yes on s and a
    press = out[2]["virial"][:3].sum() / 3 / vol                   # fix_modify virial yes on a (lj units: nktv2p = 1)
    return f, np.array(cols, dtype=np.longdouble) / n, pe, press


def a_fixture():
    with np.load(os.path.join(GOLDEN, "extforce_a.npz")) as z:
        return {k: z[k] for k in z.files}


def a_conditions(f, f0):
    """'' when the (a) case holds what it is for (told from the recorded forces and the script's own numbers)."""
    s, m = a_system(), a_members()
    fixes = a_fixes(s)
    x = a_positions()
    for k, name in enumerate(("s", "s2", "a", "z")):
        # the fix alone on the forces the fixes found (setforce: on what the three before it left)
        before = er.apply(fixes[:k], x, s["image"], s["box"], f0)[0]
        after = er.apply(fixes[:k + 1], x, s["image"], s["box"], f0)[0]
        if not (np.abs((after - before)[m[name]]).max() > 0):
            return "fix %s changes no member's force" % name
    member = m["s"] | m["s2"] | m["a"]
    for d in range(3):
        if not (s["image"][member, d] != 0).any():
            return "no member with an image flag in dimension %d" % d
    if not set(np.unique(np.abs(s["image"][member]))) >= {1, 2}:
        return "image flags of 1 and 2 are not both there"
    if not ((m["s"].astype(int) + m["s2"] + m["a"] + m["z"]) >= 2).any():
        return "no bead in two fixes"
    if not (m["z"] & (m["s"] | m["s2"])).any():
        return "the pinned group does not overlap a tethered one"
    if not (np.abs(np.asarray(f) - np.asarray(f0)).max() > 0):
        return "the fixes left the forces alone"
    return ""


def meta():
    with open(os.path.join(GOLDEN, "extforce_runs.json")) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------------------------
# (b)
# ------------------------------------------------------------------------------------------------------------------
B_N, B_SEED = 2048, 4
B_STEPS = 48
_LE = le_script(tp=0.5, n1=4, nl=5, nu=6)
_GROUPS = "group teth id 20:%d:20\ngroup pull id 10:%d:40\ngroup pinA id 7:%d:50\ngroup pinB id 33:%d:50\n" % ((B_N,) * 4)
_TETHER = "fix s teth spring/self 10.0\nfix_modify s energy yes\n"
_ADD3 = "fix a pull addforce 0.5 -0.25 0.75 every 3\nfix_modify a energy yes virial yes\n"
_ADD = "fix a pull addforce 0.5 -0.25 0.75\nfix_modify a energy yes virial yes\n"
# the crossing: bead CROSS_ID is the member of the melt closest to a face (chosen by make_extforce_runs.py, recorded in
# extforce_runs.json) and is pulled across it; it is tethered as well, so that the tether sees the image flag change
CROSS_PULL = 5.0


def _before_langevin(script, lines):
    return script.replace("fix 2 all langevin", lines + "fix 2 all langevin")


def _scn(name, script, ext_columns, fixes=rr.LE3, idle=(), point=""):
    return dict(name=name, system=dict(n=B_N, seed=B_SEED, types=("barrier", 5, 0.3)), script=script, checkpoints=[B_STEPS], fixes=fixes,
                idle=idle, point=point, ext_columns=ext_columns, family=None, contrast=None, min_ext=3)


def crossing_lines(bead, dim, sign):
    f = [0.0, 0.0, 0.0]
    f[dim] = sign * CROSS_PULL
    return ("group cross id %d\ngroup edge id %d %d\nfix s edge spring/self 2.0\nfix_modify s energy yes\n"
            "fix a cross addforce %.17g %.17g %.17g\nfix_modify a energy yes virial yes\n" % (bead, bead, bead % B_N + 1, f[0], f[1], f[2]))


def crossing_script(bead, dim, sign):
    return _LE + crossing_lines(bead, dim, sign) + "run %d\n" % B_STEPS


def _crossing_from_meta():
    try:
        c = meta()["scenarios"]["crossing"]["crossing"]
        return crossing_script(c["bead"], c["dim"], c["sign"])
    except (OSError, KeyError, ValueError):
        return None        # (not recorded yet: the generator fills the script in)


SCENARIOS = [
    _scn("tether_behind", _LE + _GROUPS + _TETHER + "run %d\n" % B_STEPS, ("pe", "f_s")),
    _scn("tether_ahead", _before_langevin(_LE, _GROUPS + _TETHER) + "run %d\n" % B_STEPS, ("pe", "f_s")),
    _scn("add_every3", _LE + _GROUPS + _ADD3 + _TETHER + "run %d\n" % B_STEPS, ("pe", "f_s", "f_a", "f_a[1]", "f_a[2]", "f_a[3]")),
    _scn("setforce", _before_langevin(_LE, _GROUPS + "fix z0 pinA setforce 0 0 0\n") + "fix z1 pinB setforce 0 0 0\nrun %d\n" % B_STEPS,
         ("f_z0[1]", "f_z0[2]", "f_z0[3]", "f_z1[1]", "f_z1[2]", "f_z1[3]")),
    _scn("tether_between", _LE + _GROUPS + "run %d\n" % (B_STEPS // 2) + _TETHER + "run %d\n" % (B_STEPS // 2), ()),
    _scn("respa2", _LE + _GROUPS + _TETHER + _ADD + "run_style respa 2 4\nrun %d\n" % B_STEPS, ("pe", "f_s", "f_a"), idle=("loop",)),
    _scn("crossing", _crossing_from_meta(), ("pe", "f_s", "f_a")),
]
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]


def b_system(scn, recorded=None):
    return rr.build_system(scn, recorded=recorded)


def thermo_columns(scn):
    return rr.thermo_columns(scn) + tuple(scn["ext_columns"])


def record_lines(scn, prefix, every):
    """rr.record_lines with the fixes' columns behind the others."""
    return rr.record_lines(scn, prefix, every).replace("thermo_style custom " + " ".join(rr.thermo_columns(scn)),
                                                       "thermo_style custom " + " ".join(thermo_columns(scn)))


def reference_script(scn, prefix, every):
    """The recording lines go in front of the first run; a fix defined between two runs (tether_between) may be named in the
    thermo line only once it exists, so that scenario records no column of it."""
    lines = scn["script"].split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("run_style"))
    return "\n".join(lines[:k]) + "\n" + record_lines(scn, prefix, every) + "\n".join(lines[k:])


class Fixture(rr.Fixture):
    def __init__(self, name):
        self.name, self.scn = name, BY_NAME[name]
        with np.load(os.path.join(GOLDEN, "extforce_b_%s.npz" % name)) as z:
            self.z = {k: z[k] for k in z.files}
        self.meta = meta()["scenarios"][name]
        self.error = self.error_step = None
        self.checkpoints = [int(c) for c in self.z["checkpoints"]]
        self.last = self.checkpoints[-1]
        self.columns = thermo_columns(self.scn)

    def system(self):
        return b_system(self.scn, recorded=self.z)

    def system_box(self):
        return rr.lattice_start(B_N, 1, B_SEED)["box"]


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def fixture_conditions(fx):
    """'' when the scenario's fixture holds what it is for: the LE fixes acted (or were idle), extruder bonds exist, every
    recorded column of the fixes is non-zero in some row, and - the crossing - an image flag of a member changes inside the
    recorded window with a list build behind the change."""
    th = fx.thermo()
    for fid in fx.scn["fixes"]:
        acted = max(th[:, fx.col("f_%s[1]" % fid)].max(), th[:, fx.col("f_%s[2]" % fid)].max()) > 0
        if acted == (fid in fx.scn["idle"]):
            return "fix %s %s" % (fid, "acted" if acted else "never acted")
    rows = fx.rows_at(fx.last)
    if (rows[:, 0] == 2).sum() < fx.scn["min_ext"]:
        return "%d type-2 bonds at the end" % (rows[:, 0] == 2).sum()
    for nm in fx.scn["ext_columns"]:
        if nm != "pe" and not (np.abs(th[:, fx.col(nm)]).max() > 0):
            return "column %s is zero in every row" % nm
    if fx.name == "crossing":
        c = fx.meta["crossing"]
        if not (0 < c["flag_changed_at"] < fx.last):
            return "no member's image flag changes inside the window"
        if not c["builds_after_change"] > 0:
            return "no list build follows the change of the image flag"
    return ""
