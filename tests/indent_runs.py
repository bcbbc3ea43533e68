"""The scenarios of the recorded reference runs with fix indent (tests/golden/indent_*.npz, indent_runs.json) and what the tests
need to read them.  tests/golden/make_indent_runs.py runs the reference binary on each and stores numbers only; test_indent_cpu.py
holds indent_reference.py and the conditions on the fixtures to them, test_gpu_indent.py the HIP path.

(a) `run 0` on the 343-bead jittered lattice of wall_runs.a_system, K = 7.5, twelve indenters (A_CASES): forces with and without
    the indenter, f_ID, f_ID[1..3] and pe of two `run 0`, without and with fix_modify energy yes.
(b) 48 steps of the LE cycle of reference_runs.py (cycle_tp05) from the prepared globule of wall_runs.b_system, with an indenter
    whose geometry is a formula of the step (ramp, vdisplace) or constant; the radii come from the start's own radial
    distribution (b_params), so that the conditions below hold.
(c) one minimisation of the globule inside a static sphere-in indenter (min_style cg, fix_modify energy yes), in the format of
    the minimize_*.npz fixtures (minimize_runs.py).
"""
import functools
import json
import os

import numpy as np

import indent_reference as ir
import reference_runs as rr
import wall_runs as wl
from systems import CHAIN_SCRIPT, le_script

GOLDEN = rr.GOLDEN
A_K = 7.5
A_THERMO = ("step", "pe", "f_c", "f_c[1]", "f_c[2]", "f_c[3]")


def a_system():
    return wl.a_system()


def _a_cases():
    L = float(a_system()["box"][0][1])
    c = 0.5 * L
    g = "%.17g"
    return {
        # a ball in the middle of the lattice
        "sphere_out": ("all", ("sphere " + g + " " + g + " " + g + " 2.5 side out") % (c, c, c)),
        # every bead inside at first sight; the radius is below the distance of the lattice's corners
        "sphere_in": ("all", ("sphere " + g + " " + g + " " + g + " 4.5 side in") % (c, c, c)),
        # the same ball as written from the neighbouring periodic images: Domain::remap brings the centre back
        "sphere_remap": ("all", ("sphere " + g + " " + g + " " + g + " 2.2 side out") % (c + L, c - L, c + 2 * L)),
        # a ball at the face x = 0: it reaches the beads below x = L through the periodic face
        "sphere_face": ("all", ("sphere 0.3 " + g + " " + g + " 2.0") % (c, c)),
        "cylinder_x": ("all", ("cylinder x " + g + " " + g + " 2.0 side out") % (c, c)),
        # (an axis at the face x = 0, as the ball above)
        "cylinder_y": ("all", ("cylinder y 0.4 " + g + " 1.8") % c),
        "cylinder_z_in": ("all", ("cylinder z " + g + " " + g + " 3.2 side in") % (c, c)),
        "cylinder_z_out": ("all", ("cylinder z " + g + " " + g + " 1.5 side out units box") % (c, c)),
        "plane_x": ("all", "plane x 2.0 lo"),
        "plane_y_lo": ("all", "plane y 1.3 lo units lattice"),
        "plane_z_hi": ("all", ("plane z " + g + " hi") % (L - 1.6)),
        # every third bead of the chain; its neighbours along the chain are inside the ball too
        "group": ("third", ("sphere " + g + " " + g + " " + g + " 2.8 side out") % (c, c, c)),
    }


A_CASES = _a_cases()
A_GROUP = "group third id 1:%d:3\n" % wl.A_N


def a_member(case):
    n = wl.A_N
    return np.ones(n, dtype=bool) if A_CASES[case][0] == "all" else (np.arange(n) % 3 == 0)


def a_indenter(case):
    return ir.parse(("indent %.17g " % A_K + A_CASES[case][1]).split())


def a_script(case):
    """What the engine runs for one (a) case: `run 0` with fix_modify at its default, then with energy yes.  None: no indenter."""
    s = CHAIN_SCRIPT + "fix 1 all nve\n"
    if case is None:
        return s + "thermo_style custom step pe\nrun 0\n"
    grp, geo = A_CASES[case]
    return s + (A_GROUP if grp != "all" else "") + ("fix c %s indent %.17g %s\nthermo_style custom %s\nrun 0\nfix_modify c energy yes\nrun 0\n"
                                                    % (grp, A_K, geo, " ".join(A_THERMO)))


def a_conditions(case):
    """'' when the case holds what it is for: at least 8 members with dr < 0 and 8 with dr >= 0; the periodic-face cases reach at
    least 4 beads through a minimum image that is not the raw difference; the remap case has its centre written outside the box;
    in the group case a non-member lies inside the indenter's reach."""
    s = a_system()
    o, member = a_indenter(case), a_member(case)
    t = ir.terms(s["x"], o, s["box"], member)
    touched, free = int(t["touched"].sum()), int((member & ~t["touched"]).sum())
    if touched < 8 or free < 8:
        return "%d members with dr < 0, %d with dr >= 0" % (touched, free)
    if case in ("sphere_face", "cylinder_y") and int(t["shifted"].sum()) < 4:
        return "%d touched beads through the periodic face" % int(t["shifted"].sum())
    if case == "sphere_remap":
        box = np.asarray(s["box"])
        if not any(o["ctr"][d] < box[d, 0] or o["ctr"][d] >= box[d, 1] for d in range(3)):
            return "the centre is written inside the box"
    if case == "group" and not ir.terms(s["x"], o, s["box"], ~member)["touched"].any():
        return "no non-member inside the indenter's reach"
    return ""


def a_fixture():
    """-> dict: f0 (no indenter), pe0, and per case f_<case> and rows_<case> (2, 6): the thermo rows of the two `run 0`."""
    with np.load(os.path.join(GOLDEN, "indent_a.npz")) as z:
        return {k: z[k] for k in z.files}


def meta():
    with open(os.path.join(GOLDEN, "indent_runs.json")) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------------------------
# (b): the LE cycle with an indenter that moves
# ------------------------------------------------------------------------------------------------------------------
B_STEPS = wl.B_STEPS
B_DT = 0.005
B_K = 10.0
INDENT_COLUMNS = ("pe", "f_c", "f_c[1]", "f_c[2]", "f_c[3]")


def b_system(recorded=None):
    return wl.b_system(recorded)


def _q(v, q):
    """A quantile of the start, rounded to 1e-3 so that the script's text is short and the same everywhere."""
    return float(np.round(np.quantile(np.asarray(v, dtype=np.float64), q), 3))


@functools.lru_cache(maxsize=None)
def b_params():
    """The geometry of the (b) and (c) indenters from the start's own distribution: radii and positions at quantiles of the
    beads' distance from the centre (sphere), from the axis (cylinder, members only), along x (plane), from the obstacle."""
    s = b_system()
    x, c = np.asarray(s["x"], dtype=np.float64), wl.b_centre()
    r = np.sqrt(((x - c[None, :]) ** 2).sum(axis=1))
    low = wl.group_low(s["type"])
    rc = np.sqrt(((x[low, :2] - c[None, :2]) ** 2).sum(axis=1))
    # the obstacle starts 2.5 from the centre and moves along +x at speed 2: 0.48 in 48 steps
    ob0, obv = float(np.round(c[0] - 2.5, 3)), 2.0
    mid = np.array([ob0 + obv * 0.5 * B_STEPS * B_DT, c[1], c[2]])
    rob = np.sqrt(((x - mid[None, :]) ** 2).sum(axis=1))
    return dict(centre=tuple(float(v) for v in c), shrink=(_q(r, 0.95), _q(r, 0.70)), piston=(_q(x[:, 0], 0.95), _q(x[:, 0], 0.88)),
                cylinder=_q(rc, 0.85), obstacle=(ob0, obv, _q(rob, 0.10)), minimize=_q(r, 0.85))


def _indent(kind, K=B_K, group="all", before_langevin=False, **geo):
    return dict(kind=kind, K=K, group=group, before_langevin=before_langevin, **geo)


def _shrink(**kw):
    p = b_params()
    return _indent("sphere", side="in", ctr=p["centre"], R=("ramp",) + p["shrink"], **kw)


def indent_lines(ind):
    """The variable and fix lines of one indenter (fix ID c)."""
    out, words = [], []

    def value(name, v):
        if isinstance(v, tuple):
            out.append("variable %s equal %s(%.17g,%.17g)" % (name, v[0], v[1], v[2]))
            return "v_" + name
        return "%.17g" % v

    if ind["kind"] == "plane":
        words = ["plane", "xyz"[ind["dim"]], value("P", ind["pos"]), "hi" if ind["planeside"] > 0 else "lo"]
    else:
        ctr = [value("XYZ"[d] + "c", ind["ctr"][d]) for d in range(3)]
        if ind["kind"] == "cylinder":
            words = ["cylinder", "xyz"[ind["dim"]]] + [ctr[d] for d in range(3) if d != ind["dim"]]
        else:
            words = ["sphere"] + ctr
        words += [value("R", ind["R"]), "side", ind["side"]]
    out.append("fix c %s indent %.17g %s units box" % (ind["group"], ind["K"], " ".join(words)))
    out.append("fix_modify c energy yes")
    return "\n".join(out) + "\n"


def geometry_at(ind, step, begin, end):
    """The indenter of indent_reference.terms at one step of a run from `begin` to `end`: ramp and vdisplace as
    src/variable.cpp evaluates them."""
    def value(v):
        if not isinstance(v, tuple):
            return float(v)
        if v[0] == "ramp":
            delta = float(step - begin)
            if delta != 0.0:
                delta /= float(end - begin)
            return v[1] + delta * (v[2] - v[1])
        return v[1] + v[2] * float(step - begin) * B_DT

    o = dict(kind=ind["kind"], K=ind["K"])
    if ind["kind"] == "plane":
        o.update(dim=ind["dim"], pos=value(ind["pos"]), planeside=ind["planeside"])
    else:
        o.update(ctr=[value(v) for v in ind["ctr"]], R=value(ind["R"]), side=ind["side"], dim=ind.get("dim", 0))
    return o


def geometry_values(o):
    return np.array(list(o.get("ctr", [])) + [o.get("R", 0.0), o.get("pos", 0.0)], dtype=np.float64)


_LE = le_script(tp=0.5, n1=4, nl=5, nu=6)
_WALL = wl.b_region() + "fix w all wall/region ball lj126 1.0 1.0 %.17g\n" % wl.B_CUT


def _script(ind, head=_LE, extra="", runs=(B_STEPS,), tail=""):
    lines = indent_lines(ind)
    if ind["group"] != "all":
        lines = "group low type 1 2\n" + lines
    s = head.replace("fix 2 all langevin", lines + "fix 2 all langevin") if ind["before_langevin"] else head + lines
    return s + extra + "".join("run %d\n" % n for n in runs) + tail


def _scn(name, ind, point="", idle=(), variable=True, **kw):
    runs = kw.get("runs", (B_STEPS,))
    return dict(name=name, system=dict(n=wl.B_N), script=_script(ind, **kw), checkpoints=[B_STEPS], fixes=rr.LE3, idle=idle, point=point,
                indent=ind, runs=tuple(runs), variable=variable, family=None, contrast=None, min_ext=3)


def _scenarios():
    p = b_params()
    c = p["centre"]
    ob0, obv, obr = p["obstacle"]
    return [
        _scn("shrink", _shrink()),
        _scn("shrink_before_langevin", _shrink(before_langevin=True)),
        _scn("obstacle", _indent("sphere", K=1.0, side="out", ctr=(("vdisplace", ob0, obv), c[1], c[2]), R=obr)),
        _scn("piston", _indent("plane", K=2.0, dim=0, planeside=1, pos=("ramp",) + p["piston"])),
        _scn("cyl_group", _indent("cylinder", group="low", dim=2, side="in", ctr=c, R=p["cylinder"]), variable=False),
        _scn("sort3", _shrink(), head=_LE.replace("atom_modify sort 0 0", "atom_modify sort 3 0"), point="sorted"),
        _scn("respa2", _shrink(), extra="run_style respa 2 4\n", idle=("loop",)),
        _scn("with_wall", _shrink(), head=_LE + _WALL),
        _scn("two_runs", _shrink(), runs=(B_STEPS // 2, B_STEPS // 2), tail="unfix c\n"),
    ]


SCENARIOS = _scenarios()
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]


def thermo_columns(scn):
    return rr.thermo_columns(scn) + INDENT_COLUMNS


def record_lines(scn, prefix, every):
    """rr.record_lines with the indenter's columns behind the others."""
    return rr.record_lines(scn, prefix, every).replace("thermo_style custom " + " ".join(rr.thermo_columns(scn)),
                                                       "thermo_style custom " + " ".join(thermo_columns(scn)))


def first_run_line(lines):
    return next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("run_style"))


def reference_script(scn, prefix, every):
    lines = scn["script"].split("\n")
    k = first_run_line(lines)
    return "\n".join(lines[:k]) + "\n" + record_lines(scn, prefix, every) + "\n".join(lines[k:])


def run_of_step(scn, step):
    """(begin, end) of the run command that holds `step` (the later run at a boundary, as the set-up of that run evaluates it -
    except the very last step, which belongs to the last run)."""
    begin = 0
    for n in scn["runs"]:
        if step < begin + n or begin + n == sum(scn["runs"]):
            return begin, begin + n
        begin += n
    raise ValueError(step)


class Fixture(rr.Fixture):
    def __init__(self, name):
        self.name, self.scn = name, BY_NAME[name]
        with np.load(os.path.join(GOLDEN, "indent_b_%s.npz" % name)) as z:
            self.z = {k: z[k] for k in z.files}
        self.meta = meta()["scenarios"][name]
        self.checkpoints = [int(c) for c in self.z["checkpoints"]]
        self.last = self.checkpoints[-1]
        self.columns = thermo_columns(self.scn)

    def system(self):
        return b_system(recorded=self.z)

    def system_box(self):
        return wl.b_box()


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def member_of(scn, types):
    return wl.group_low(types) if scn["indent"]["group"] != "all" else np.ones(len(types), dtype=bool)


def touched_fraction(scn, x, types, step):
    begin, end = run_of_step(scn, step)
    member = member_of(scn, types)
    t = ir.terms(x, geometry_at(scn["indent"], step, begin, end), wl.b_box(), member)
    return float(t["touched"].sum()) / float(member.sum())


def fixture_conditions(fx):
    """'' when the scenario's fixture holds what it is for: the LE part of wall_runs.fixture_conditions (the LE fixes acted or were
    idle, extruder bonds exist at the end), at least 5 % of the indenter's members have dr < 0 at the last step, a variable
    geometry ends more than 0.05 from where it began, f_c is non-zero in every thermo row, and the scenario's own point."""
    th, scn = fx.thermo(), fx.scn
    for fid in scn["fixes"]:
        acted = max(th[:, fx.col("f_%s[1]" % fid)].max(), th[:, fx.col("f_%s[2]" % fid)].max()) > 0
        if acted == (fid in scn["idle"]):
            return "fix %s %s" % (fid, "acted" if acted else "never acted")
    rows = fx.rows_at(fx.last)
    if (rows[:, 0] == 2).sum() < scn["min_ext"]:
        return "%d type-2 bonds at the end" % (rows[:, 0] == 2).sum()
    frac = touched_fraction(scn, fx.z["x"][-1], fx.z["type"][-1], fx.last)
    if frac < 0.05:
        return "only %.3f of the members with dr < 0 at the last step" % frac
    if scn["variable"]:
        first = geometry_values(geometry_at(scn["indent"], 0, *run_of_step(scn, 0)))
        last = geometry_values(geometry_at(scn["indent"], fx.last, *run_of_step(scn, fx.last)))
        if not np.abs(last - first).max() > 0.05:
            return "the geometry moved by %.3g" % np.abs(last - first).max()
    if not (np.abs(th[:, fx.col("f_c")]) > 0).all():
        return "f_c is zero in a thermo row"
    if scn["point"] == "sorted" and not (fx.z["local_order"] != np.arange(1, len(fx.z["local_order"]) + 1)).any():
        return "Atom::sort left the order alone"
    return ""


# ------------------------------------------------------------------------------------------------------------------
# (c): the globule minimised inside a static sphere-in indenter
# ------------------------------------------------------------------------------------------------------------------
C_NAME = "indent"
C_COLUMNS = ("f_c", "f_c[1]", "f_c[2]", "f_c[3]")


def c_indenter():
    p = b_params()
    return _indent("sphere", side="in", ctr=p["centre"], R=p["minimize"])


def c_scenario():
    """The scenario in the form of minimize_runs.SCENARIOS (its script(), columns() and parse_log() read it)."""
    return dict(name=C_NAME, modify="", head=CHAIN_SCRIPT, before=indent_lines(c_indenter()), minimize="minimize 0 0 24 10000", thermo=4,
                system=dict(n=wl.B_N), extra_columns=C_COLUMNS, after="")


def c_system():
    return b_system()


def c_fixture():
    import minimize_runs as mn
    fx = mn.Fixture.__new__(mn.Fixture)
    fx.name, fx.scn = C_NAME, c_scenario()
    with np.load(os.path.join(GOLDEN, "indent_c.npz")) as z:
        fx.z = {k: z[k] for k in z.files}
    fx.meta = meta()["c"]
    fx.columns = mn.columns(fx.scn)
    return fx


def c_conditions(fx):
    """'' when the minimisation holds what it is for: at least 5 % of the beads touch the indenter at the start, its energy is in
    pe (fix_modify energy yes) and non-zero in every row, the energy never rises, and the run ends at its iteration limit."""
    t = ir.terms(c_system()["x"], geometry_at(c_indenter(), 0, 0, 1), wl.b_box())
    if float(t["touched"].mean()) < 0.05:
        return "only %.3f of the beads touch the indenter at the start" % float(t["touched"].mean())
    th = fx.z["thermo"]
    if not (np.abs(th[:, fx.col("f_c")]) > 0).all():
        return "f_c is zero in a thermo row"
    share = th[0, fx.col("pe")] - (th[0, fx.col("epair")] + th[0, fx.col("emol")])
    if abs(share - th[0, fx.col("f_c")]) > 1e-12 * max(1.0, abs(share)):
        return "pe holds %.17g of the fix, f_c reports %.17g" % (share, th[0, fx.col("f_c")])
    if (np.diff(th[:, fx.col("pe")]) > 0).any():
        return "the energy rises from one row to the next"
    st = fx.stats()
    if int(st["stop"]) != 0 or int(st["iterations"]) != 24:
        return "stop %d after %d iterations" % (st["stop"], st["iterations"])
    return ""
