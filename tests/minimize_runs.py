"""The scenarios of the recorded reference minimisations (tests/golden/minimize_<name>.npz, minimize_runs.json) and what the tests
need to read them.  tests/golden/make_minimize_runs.py runs the reference binary on each and stores numbers only;
test_minimize_cpu.py holds the conditions on the fixtures, test_gpu_minimize.py the HIP path.

Every scenario starts from the 1000-bead melt of reference_runs (box 10.56, more than three neighbour cutoffs) under the chain
script of systems.py, whose `neigh_modify every 1 delay 1 check yes` differs from what a minimisation uses: each run prints the
warning and restores the setting.  The stop string is held as its index into STOP_STRINGS.
"""
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reference_runs as rr
from systems import CHAIN_SCRIPT, ANGLE_SCRIPT, le_script

GOLDEN = rr.GOLDEN
FACTOR = rr.FACTOR
N, SEED = 1000, 1
COLUMNS = ("step", "temp", "pe", "epair", "emol", "press", "fmax", "fnorm")
from lammps_le_amd import MIN_STOP_STRINGS as STOP_STRINGS      # noqa: E402  (one table: the package's)
MAXITER, MAXEVAL, ETOL, FTOL, DOWNHILL, ZEROALPHA, ZEROFORCE, ZEROQUAD = range(8)
STAT_KEYS = ("stop", "e_initial", "e_previous", "e_final", "fnorm_initial", "fnorm_final", "fmax_initial", "fmax_final", "alpha", "max_move",
             "iterations", "evals", "steps")


def meta():
    with open(os.path.join(GOLDEN, "minimize_runs.json")) as fh:
        return json.load(fh)


def _box():
    b = np.asarray(rr.lattice_start(N, 1, SEED)["box"], dtype=np.float64)
    return b


def _confined():
    """A sphere around the whole box with its wall felt in the corners (energy yes), tethers moved off their origins (energy
    yes), a pull every third iteration (energy yes), beads held in y and z, and a second wall without energy yes."""
    b = _box()
    c = 0.5 * (b[:, 0] + b[:, 1])
    L = float(b[0, 1] - b[0, 0])
    s = "region ball sphere %.17g %.17g %.17g %.17g side in\n" % (c[0], c[1], c[2], 0.87 * L)
    s += "region slab block %.17g %.17g %.17g %.17g %.17g %.17g side in\n" % (b[0, 0] - 0.4, b[0, 1] + 0.4, b[1, 0] - 0.4, b[1, 1] + 0.4,
                                                                               b[2, 0] - 0.4, b[2, 1] + 0.4)
    s += "group teth id 20:%d:20\ngroup pull id 10:%d:40\ngroup pin id 7:%d:50\n" % (N, N, N)
    s += "fix w all wall/region ball lj126 1.0 1.0 2.5\nfix_modify w energy yes\n"
    s += "fix w2 all wall/region slab harmonic 5.0 0.0 1.0\n"
    s += "fix s teth spring/self 10.0\nfix_modify s energy yes\n"
    # (the tethers' origins are where the fix command found the beads: five of them are then moved 0.05 towards the centre)
    x = rr.load_melt(N, 1, SEED)["x"]
    for i in range(20, N + 1, 200):
        to = x[i - 1] + 0.05 * np.sign(c - x[i - 1])
        s += "set atom %d x %.17g y %.17g z %.17g\n" % (i, to[0], to[1], to[2])
    s += "fix a pull addforce 0.5 -0.25 0.75 every 3\nfix_modify a energy yes\n"
    s += "fix z pin setforce NULL 0 0\n"
    return s


_ANGLES = ANGLE_SCRIPT + "angle_style cosine\nangle_coeff 1 2.0\nangle_coeff 2 2.0\n"


def _scn(name, minimize, before="", thermo=5, head=CHAIN_SCRIPT, system=None, extra_columns=(), modify="", after=""):
    return dict(name=name, modify=modify, head=head, before=before, minimize=minimize, thermo=thermo, system=system or dict(n=N, seed=SEED),
                extra_columns=tuple(extra_columns), after=after)


# soft_overlap: a 300-bead phantom walk (freely overlapping) under pair_style soft with A = 30
SOFT_N, SOFT_SEED = 300, 3
_SOFT = CHAIN_SCRIPT.replace("pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12\n", "pair_style soft 1.12246\npair_coeff * * 30.0\n")
assert "soft" in _SOFT
# then_run: the three LE fixes, fix nve and fix langevin defined before the minimisation, Atom::sort every 5 steps
THEN_ITER, THEN_RUN = 12, 24
_THEN = le_script(tp=0.5, n1=4, nl=5, nu=6).replace("atom_modify sort 0 0", "atom_modify sort 5 0")
assert "sort 5 0" in _THEN
LE_COLUMNS = ("bonds",) + tuple("f_%s[%d]" % (f, k) for f in rr.LE3 for k in (1, 2))


def _crossing_before():
    """The bead the recorder picked (minimize_runs.json): put 0.01 inside the periodic face its force points through."""
    try:
        c = meta()["scenarios"]["crossing"]["crossing"]
    except (OSError, KeyError, ValueError):
        return None          # (not recorded yet: the generator fills it in)
    return crossing_before(c["bead"], c["dim"], c["sign"])


def crossing_before(bead, dim, sign):
    b = _box()
    return "set atom %d %s %.17g\n" % (bead, "xyz"[dim], (b[dim, 1] - 0.01) if sign > 0 else (b[dim, 0] + 0.01))


SCENARIOS = [
    _scn("cg_default", "minimize 0 0 30 10000"),
    _scn("sd_backtrack", "minimize 0 0 30 10000", "min_style sd\nmin_modify line backtrack\n"),
    _scn("stop_etol", "minimize 1.0e-3 0 40 10000"),
    _scn("stop_ftol_two", "minimize 0 60.0 40 10000"),
    _scn("stop_ftol_max", "minimize 0 12.0 40 10000", "min_modify norm max\n"),
    _scn("stop_ftol_inf", "minimize 0 10.0 40 10000", "min_modify norm inf\n"),
    _scn("stop_maxeval", "minimize 0 0 40 25"),
    _scn("stop_zeroforce", "minimize 0 0 30 10000", "fix z all setforce 0 0 0\n"),
    _scn("dmax_small", "minimize 0 0 20 10000", "min_modify dmax 0.02\n"),
    _scn("confined_tethered", "minimize 0 0 24 10000", _confined(), thermo=3, extra_columns=("f_w", "f_w2", "f_s", "f_a")),
    _scn("angles", "minimize 0 0 20 10000", head=_ANGLES, system=dict(n=N, nchains=2, seed=6, angles=True), extra_columns=("eangle",)),
    _scn("soft_overlap", "minimize 0 0 30 10000", head=_SOFT, system=dict(n=SOFT_N, seed=SOFT_SEED, phantom=True)),
    _scn("crossing", "minimize 0 0 32 10000", _crossing_before()),
    _scn("then_run", "minimize 0 0 %d 1000" % THEN_ITER, head=_THEN, thermo=4, system=dict(n=N, seed=SEED, types=("barrier", 5, 0.3)),
         extra_columns=LE_COLUMNS, after="run %d\n" % THEN_RUN),
    _scn("norm_no", "minimize 0 0 30 10000", modify="thermo_modify norm no\n"),      # (behind thermo_style, which starts the settings over)
]
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]


def columns(scn):
    return COLUMNS + scn["extra_columns"]


def system(scn):
    if scn["system"].get("phantom"):
        from lammps_le_amd.synth import phantom_chains
        s = phantom_chains(scn["system"]["n"], 1, 0.85, seed=scn["system"]["seed"])
        s["nbondtypes"] = 2
        return s
    recorded = None
    if scn["system"].get("types") is not None:      # (types drawn from a random stream: the tests take the recorded ones)
        try:
            with np.load(os.path.join(GOLDEN, "minimize_%s.npz" % scn["name"])) as z:
                recorded = dict(start_type=z["start_type"])
        except OSError:
            pass
    return rr.build_system(dict(system=scn["system"]), recorded=recorded)


def script(scn, fmt=True):
    """The scenario's script up to and including the minimisation (read_data names data.chain)."""
    s = scn["head"] + scn["before"]
    s += "thermo_style custom %s\n" % " ".join(columns(scn)) + scn["modify"]
    if fmt:
        s += "thermo_modify format float %.17g\n"
    s += "thermo %d\n" % scn["thermo"] + scn["minimize"] + "\n"
    return s


def closest_pair(x, scn):
    from soft_runs import closest_nonbonded
    s = system(scn)
    return closest_nonbonded(x, s["box"], s["bonds"])


def minimize_args(scn):
    w = scn["minimize"].split()
    return float(w[1]), float(w[2]), int(w[3]), int(w[4])


_NUM = r"([-+0-9.eEinfa]+)"


def parse_log(text, ncol):
    """Thermo rows and the stats block (src/finish.cpp:196-216 layout) of a log that holds ONE minimisation."""
    rows = []
    for ln in text.split("\n"):
        w = ln.split()
        if len(w) == ncol and re.match(r"^\d+$", w[0]):
            try:
                rows.append([float(v) for v in w])
            except ValueError:
                pass
    st = {}
    m = re.search(r"Stopping criterion = (.*)", text)
    st["stop"] = STOP_STRINGS.index(m.group(1).strip())
    m = re.search(r"Energy initial, next-to-last, final = \s*\n\s*" + _NUM + r"\s+" + _NUM + r"\s+" + _NUM, text)
    st["e_initial"], st["e_previous"], st["e_final"] = (float(v) for v in m.groups())
    m = re.search(r"Force two-norm initial, final = " + _NUM + " " + _NUM, text)
    st["fnorm_initial"], st["fnorm_final"] = (float(v) for v in m.groups())
    m = re.search(r"Force max component initial, final = " + _NUM + " " + _NUM, text)
    st["fmax_initial"], st["fmax_final"] = (float(v) for v in m.groups())
    m = re.search(r"Final line search alpha, max atom move = " + _NUM + " " + _NUM, text)
    st["alpha"], st["max_move"] = (float(v) for v in m.groups())
    m = re.search(r"Iterations, force evaluations = (\d+) (\d+)", text)
    st["iterations"], st["evals"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"Loop time of \S+ on \d+ procs for (\d+) steps", text)
    st["steps"] = int(m.group(1))
    st["builds"] = [int(v) for v in re.findall(r"Neighbor list builds = (\d+)", text)]
    st["warned"] = "Using 'neigh_modify every 1 delay 0 check yes' setting during minimization" in text
    return np.array(rows), st


class Fixture:
    def __init__(self, name):
        self.name, self.scn = name, BY_NAME[name]
        with np.load(os.path.join(GOLDEN, "minimize_%s.npz" % name)) as z:
            self.z = {k: z[k] for k in z.files}
        self.meta = meta()["scenarios"][name]
        self.columns = columns(self.scn)

    def col(self, name):
        return self.columns.index(name)

    def stats(self):
        return dict(zip(STAT_KEYS, self.z["stats"]))


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def conditions(fx):
    """'' when the fixture holds what its scenario is for."""
    st, th, name = fx.stats(), fx.z["thermo"], fx.name
    etol, ftol, maxiter, maxeval = minimize_args(fx.scn)
    it, stop = int(st["iterations"]), int(st["stop"])
    if it > 40:
        return "%d iterations" % it
    if name == "then_run":
        th = th[:int(np.nonzero(th[:, 0] == it)[0][0]) + 1]          # (the rows of the minimisation; the run's follow)
    if th[0, 0] != 0 or th[-1, 0] != it:
        return "thermo rows do not run from the set-up to the last iteration"
    pe = th[:, fx.col("pe")]
    if (np.diff(pe) > 0).any():
        return "the energy rises from one row to the next"
    want = dict(stop_etol=ETOL, stop_ftol_two=FTOL, stop_ftol_max=FTOL, stop_ftol_inf=FTOL, stop_maxeval=MAXEVAL)
    if name in want:
        if stop != want[name] or not 0 < it < maxiter:
            return "stop %d after %d of %d iterations" % (stop, it, maxiter)
    elif name == "stop_zeroforce":
        # with every force zero the line search leaves at its first test, f.h <= 0 (src/min_linesearch.cpp:351), ahead of the
        # test on max |h| (:382): the reference's words for this state are `search direction is not downhill`, in iteration 1
        if stop != DOWNHILL or it != 1 or int(st["evals"]) != 0 or st["fnorm_initial"] != 0.0:
            return "stop %d, %d iterations, %d evaluations, |f| %g" % (stop, it, st["evals"], st["fnorm_initial"])
    elif stop != MAXITER or it != maxiter:
        return "stop %d after %d of %d iterations" % (stop, it, maxiter)
    if name == "dmax_small" and not fx.meta["alpha_is_alphamax"]:
        return "the final alpha is never alphamax"
    if name == "confined_tethered":
        for c in fx.scn["extra_columns"]:
            if not abs(th[0, fx.col(c)]) > 0:
                return "column %s is zero at the start" % c
        share = th[0, fx.col("pe")] - (th[0, fx.col("epair")] + th[0, fx.col("emol")])
        want_share = th[0, fx.col("f_w")] + th[0, fx.col("f_s")] + th[0, fx.col("f_a")]
        if not abs(share) > 0 or abs(share - want_share) > 1e-12 * max(1.0, abs(share)):
            return "pe holds %.17g of the fixes, the energy-yes fixes report %.17g" % (share, want_share)
    if name == "angles" and not (th[:, fx.col("eangle")] > 0).all():
        return "no angle energy"
    if name == "soft_overlap":
        c = fx.meta["closest"]
        if not (c["start"] < 0.3 and c["end"] > c["start"]):
            return "closest pair %.3f at the start, %.3f at the end" % (c["start"], c["end"])
    if name == "crossing":
        c = fx.meta["crossing"]
        if not (0 < c["flag_changed_at"] < it) or not fx.z["builds"][0] > 0:
            return "the bead's image flag does not change inside the minimisation"
    if name == "then_run":
        t = fx.meta["then_run"]
        if not t["sorted_inside"]:
            return "no Atom::sort inside the minimisation"
        if t["bonds_changed_in_min"] or not t["first_bond_change"] > it:
            return "the bond rows change inside the minimisation, or never"
        full = fx.z["thermo"]
        if full[-1, 0] != it + THEN_RUN or not max(full[-1, fx.col("f_loop[2]")], full[-1, fx.col("f_loading[2]")]) > 0:
            return "the run does not continue the step count, or no LE fix fired in it"
    if name == "norm_no" and not abs(th[0, fx.col("pe")]) > 100:
        return "the energies look normalised"
    if not fx.meta["warned"]:
        return "the neigh_modify warning is missing"
    return ""


# ------------------------------------------------------------------------------------------------------------------
# the engine's side
# ------------------------------------------------------------------------------------------------------------------
def run_engine(scn, tmp_path, before_script=None, keep=False):
    """The scenario through the C-ABI -> dict(thermo rows, stats block, x f image by ID, local order, counters, log text)."""
    from systems import run_product
    log = os.path.join(str(tmp_path), "log.%s" % scn["name"])
    p = run_product(script(scn), system(scn), tmp_path, cmdargs=("-screen", "none", "-log", log))
    try:
        text = open(log).read()
        rows, st = parse_log(text, len(columns(scn)))
        stat = {k: p.stat(k) for k in ("min_iterations", "min_evals", "min_stop", "min_alpha", "min_host_waits", "min_rebuilds",
                                       "host_downloads", "neigh_builds")}
        got = dict(thermo=rows, stats=st, text=text, stat=stat, x=p.gather("x"), f=p.gather("f"), image=p.gather("image"),
                   local_order=np.asarray(p.gather_atoms_concat("id", 0, 1)).astype(np.int32).ravel(),
                   bonds=rr.bond_rows(p.gather("num_bond"), p.gather("bond_type"), p.gather("bond_atom")),
                   step=int(p.get_thermo("step")), pe=p.get_thermo("pe"), fmax=p.get_thermo("fmax"), fnorm=p.get_thermo("fnorm"))
        if scn["after"]:
            for ln in scn["after"].split("\n"):
                p.command(ln)
            rows2, _ = parse_log(open(log).read(), len(columns(scn)))
            got["after"] = dict(thermo=rows2, x=p.gather("x"), v=p.gather("v"), image=p.gather("image"),
                                local_order=np.asarray(p.gather_atoms_concat("id", 0, 1)).astype(np.int32).ravel(),
                                bonds=rr.bond_rows(p.gather("num_bond"), p.gather("bond_type"), p.gather("bond_atom")),
                                fixvec={f: (p.extract_fix(f, 0, 1, 0), p.extract_fix(f, 0, 1, 1)) for f in rr.LE3},
                                steps_fused=p.stat("steps_fused"), step=int(p.get_thermo("step")))
    except Exception:
        p.close()
        raise
    if keep:
        return got, p
    p.close()
    return got
