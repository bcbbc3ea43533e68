"""fix indent on the HIP path: k_indent and the indent variants of the step kernel against recorded runs of the reference binary
(tests/golden/indent_*.npz, scenario table indent_runs.py) and against the long-double restatement (indent_reference.py).
Nothing here reads the reference or its binary.

`run 0`: forces, f_ID, f_ID[k] and pe of the twelve indenters, bound 1e-12 relative to max(1, |value|) (the project's bound for
single evaluations).  The LE cycle with an indenter that moves, 48 steps: bond rows, counters, list builds, local order and image
flags exactly, x / v / f under 16 x the spread the reference shows against itself from starts moved by one ulp, thermo columns
within the bounds reference_runs derives from the same spread - in the three shapes of the step kernel and through the unfused
kernels, with the path the steps took.  One recorded minimisation, a restart in the middle of a ramp, and the allocations a
handle leaves behind."""
import os

import numpy as np
import pytest

import indent_reference as ir
import indent_runs as ind
import minimize_runs as mn
import reference_runs as rr
from systems import run_product

pytestmark = pytest.mark.gpu

RUN0_BOUND = 1e-12
PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD, "unfused": {"LAMMPS_LE_NO_FUSE": "1"}}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall", "steps_fused_indent")
CONTINUOUS = ("temp", "epair", "emol", "etotal", "press")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def last_thermo_row(log, ncol):
    rows = [w for w in (ln.split() for ln in open(log).read().split("\n")) if len(w) == ncol and w[0].isdigit()]
    return [float(v) for v in rows[-1]]


# ------------------------------------------------------------------------------------------------------------------
# run 0: k_indent<EFLAG>, the column sums, eval_thermo
# ------------------------------------------------------------------------------------------------------------------
_f0 = {}


def forces_without(tmp_path):
    if "f" not in _f0:
        p = run_product(ind.a_script(None), ind.a_system(), tmp_path)
        _f0["f"] = p.gather("f")
        p.close()
    return _f0["f"]


@pytest.mark.parametrize("case", list(ind.A_CASES))
def test_run0(tmp_path, monkeypatch, case):
    """One indenter: per-bead forces against the recorded ones, the indenter's share of them (forces with minus forces without,
    both the engine's) against indent_reference, f_ID and f_ID[1..3] (extract_fix: the sums; the thermo keyword: per atom under
    norm yes) against both, pe of the two `run 0` - fix_modify energy no, then yes - against the recorded rows."""
    set_env(monkeypatch, {})
    fx, s = ind.a_fixture(), ind.a_system()
    n = len(s["x"])
    f0 = forces_without(tmp_path)
    t = ir.terms(s["x"], ind.a_indenter(case), s["box"], ind.a_member(case))
    lines = ind.a_script(case).split("\n")
    cut = lines.index("fix_modify c energy yes")
    log = os.path.join(str(tmp_path), "log.run0")
    lines.insert(lines.index("run 0"), "thermo_modify format float %.17g")
    p = run_product("\n".join(lines[:cut + 1]), s, tmp_path, cmdargs=("-screen", "none", "-log", log))
    rows = fx["rows_" + case]
    col = ind.A_THERMO.index
    f = p.gather("f")
    figures = {"f against the recorded run": rel(f, fx["f_" + case]),
               "indenter's share against indent_reference": float((np.abs((f - f0) - t["f"].astype(np.float64)) / np.maximum(1.0, np.abs(f))).max())}
    want = [float(t["energy"])] + [float(v) for v in t["findent"]]
    for run in (0, 1):
        if run:
            p.command("fix_modify c energy yes")
            p.command("run 0")
        sums = [p.extract_fix("c", 0, 0)] + [p.extract_fix("c", 0, 1, k) for k in range(3)]
        figures["run %d f_ID sums against indent_reference" % run] = rel(sums, want)
        figures["run %d f_ID sums against the recorded rows" % run] = rel(np.array(sums) / n, rows[run][col("f_c"):col("f_c") + 4])
        figures["run %d pe" % run] = rel(p.get_thermo("pe"), rows[run][col("pe")])
        # the thermo keywords print the sums per atom (thermo_modify norm yes): the last row of the log
        printed = last_thermo_row(log, len(ind.A_THERMO))
        figures["run %d thermo keywords, per atom" % run] = rel(printed[2:], np.array(sums) / n)
    assert int(p.stat("steps_fused")) == 0
    p.close()
    bad = []
    for what, err in figures.items():
        print("%-16s %-46s %.2e" % (case, what, err))
        if not err < RUN0_BOUND:
            bad.append("%s %s: %.3e exceeds %.1e" % (case, what, err, RUN0_BOUND))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the LE cycle with a moving indenter: the recorded runs
# ------------------------------------------------------------------------------------------------------------------
def engine_run(script, system, fixes, tmp_path, indent=True, tail=""):
    lines = script.split("\n")
    lines.insert(ind.first_run_line(lines), "thermo_style custom " + " ".join(("step",) + rr.THERMO))
    p = run_product("\n".join(lines), system, tmp_path)
    try:
        nb = p.gather("num_bond")
        got = dict(bond=rr.bond_rows(nb, p.gather("bond_type"), p.gather("bond_atom")), angle=None, type=p.gather("type"),
                   image=p.gather("image"), x=p.gather("x"), v=p.gather("v"), f=p.gather("f"), bonds=float(p.get_thermo("bonds")),
                   fixvec={fid: (float(p.extract_fix(fid, 0, 1, 0)), float(p.extract_fix(fid, 0, 1, 1))) for fid in fixes},
                   builds=int(p.stat("neigh_builds")), stats={k: int(p.stat(k)) for k in STATS}, fene=int(p.stat("fene_warnings")),
                   pe=p.get_thermo("pe"), local_order=np.asarray(p.gather_atoms_concat("id", 0, 1)).astype(np.int32).ravel())
        if indent:
            got["indent"] = [p.extract_fix("c", 0, 0)] + [p.extract_fix("c", 0, 1, k) for k in range(3)]
        got["rows"] = [dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5], bonds=r[6]) for r in p.thermo_history()]
        if tail:
            p.command(tail)
        got["fix_ids"] = p.available_ids("fix")
    finally:
        p.close()
    return got


def scenario_run(name, tmp_path):
    fx = ind.fixture(name)
    script = fx.scn["script"]
    tail = ""
    if script.endswith("unfix c\n"):          # (the sums are read before the unfix; it is issued behind them)
        script, tail = script[:-len("unfix c\n")], "unfix c"
    got = engine_run(script, fx.system(), fx.scn["fixes"], tmp_path, tail=tail)
    assert ("c" in got["fix_ids"]) == (not tail)
    return got


def compare_end(name, got, label):
    fx = ind.fixture(name)
    bad = rr.check_discrete(fx, fx.last, got)
    if got["builds"] != fx.z["builds"][-1]:
        bad.append("list builds of the last run: %d against %d recorded" % (got["builds"], fx.z["builds"][-1]))
    if got["fene"] != fx.meta["fene_warnings"]:
        bad.append("FENE warnings: %d against %d recorded" % (got["fene"], fx.meta["fene_warnings"]))
    if not np.array_equal(got["local_order"], fx.z["local_order"]):
        bad.append("the local order differs from the recorded one")
    if not np.array_equal(got["image"], fx.z["image"][-1]):
        bad.append("the image flags differ from the recorded ones")
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), label)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], CONTINUOUS), label)
    if [r["bonds"] for r in got["rows"]] != list(fx.thermo()[:, fx.col("bonds")]):
        bad.append("the bonds column differs from the recorded one")
    # the last row: pe with the indenter's energy in it, f_c and f_c[1..3] (recorded per atom: thermo_modify norm yes)
    n, row = len(got["type"]), fx.thermo()[-1]
    dev = {(len(fx.thermo()) - 1, "pe"): abs(got["pe"] - row[fx.col("pe")])}
    for k, nm in enumerate(ind.INDENT_COLUMNS[1:]):
        dev[(len(fx.thermo()) - 1, nm)] = abs(got["indent"][k] / n - row[fx.col(nm)])
    bad += rr.check_thermo(fx, dev, label)
    return bad


def expected_paths(name, shape):
    """48 steps with `thermo 10`: five thermo steps, which a run with an indenter takes through the unfused kernels in every
    shape; r-RESPA and an indenter on a group are unfused altogether; two runs of 24 steps have three thermo steps each, and the
    counters are those of the second."""
    zero = dict.fromkeys(STATS, 0)
    if name == "two_runs":
        return dict(zero, steps_unfused=24) if shape == "unfused" else dict(zero, steps_fused=21, steps_fused_indent=21, steps_unfused=3)
    if shape == "unfused" or name in ("respa2", "cyl_group"):
        return dict(zero, steps_unfused=48)
    return dict(zero, steps_fused=43, steps_fused_indent=43, steps_fused_wall=43 if name == "with_wall" else 0, steps_unfused=5)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ind.NAMES)
def test_recorded_runs(tmp_path, monkeypatch, name, shape):
    """Every recorded run in the three shapes of the step kernel and through the unfused kernels.  Measured on an MI355X, the
    largest over the 36 cases: x 8.9e-15 (smallest bound 2.0e-13), v 2.3e-13 (4.9e-12), f 1.2e-11 (2.5e-10); thermo columns, pe
    and f_c[k] at most 6 % of their bounds.  `run 0` (test_run0): at most 9.5e-14 (plane_y_lo, forces against the recorded run)
    against 1e-12.  Fused against unfused (test_fused_against_unfused): x 1.7e-15, v 1.3e-13.  The minimisation: x 1.6e-14
    (bound 4.2e-13), f 2.5e-11 (4.0e-10), thermo columns at most 0.77 of their bounds."""
    set_env(monkeypatch, SHAPES[shape])
    got = scenario_run(name, tmp_path)
    bad = compare_end(name, got, "%s %s" % (name, shape))
    assert not bad, "\n".join(bad)
    assert got["stats"] == expected_paths(name, shape), got["stats"]


@pytest.mark.parametrize("name", ["shrink", "shrink_before_langevin"])
@pytest.mark.parametrize("shape", ["four", "plain", "ahead"])
def test_fused_against_unfused(tmp_path, monkeypatch, name, shape):
    """The same script through the indent variant of the step kernel and through k_indent: x to 1e-9, v to 1e-8 relative (the
    figures test_gpu_wall.py uses), the same list builds and bond rows."""
    runs = {}
    for label, env in (("fused", SHAPES[shape]), ("unfused", SHAPES["unfused"])):
        set_env(monkeypatch, env)
        runs[label] = scenario_run(name, tmp_path)
    a, b = runs["fused"], runs["unfused"]
    assert a["stats"]["steps_fused_indent"] == 43 and b["stats"]["steps_fused_indent"] == 0 and a["stats"]["steps_fused_wall"] == 0
    print("%s %s: x %.2e v %.2e" % (name, shape, rel(a["x"], b["x"]), rel(a["v"], b["v"])))
    assert rel(a["x"], b["x"]) < 1e-9 and rel(a["v"], b["v"]) < 1e-8
    assert a["builds"] == b["builds"] and np.array_equal(a["bond"], b["bond"]) and np.array_equal(a["image"], b["image"])


def _with_radius(script, text):
    """The shrink script with another definition of its radius: `text` replaces the ramp's variable line."""
    lines = script.split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("variable R equal"))
    lines[k:k + 1] = text
    return "\n".join(lines)


def test_constant_twin(tmp_path, monkeypatch):
    """A constant radius takes the same path as a variable one (the table travels with the launch either way), and the radius
    given as a number is bit for bit the radius given as v_R with `variable R equal 6.5`."""
    set_env(monkeypatch, PLAIN)
    fx = ind.fixture("shrink")
    variable = scenario_run("shrink", tmp_path)
    as_var = engine_run(_with_radius(fx.scn["script"], ["variable R equal 6.5"]), fx.system(), fx.scn["fixes"], tmp_path)
    as_num = engine_run(_with_radius(fx.scn["script"], []).replace("v_R", "6.5"), fx.system(), fx.scn["fixes"], tmp_path)
    assert as_var["stats"] == as_num["stats"] == variable["stats"], (as_var["stats"], as_num["stats"], variable["stats"])
    assert as_num["stats"]["steps_fused"] == 43
    for q in ("x", "v", "f", "image", "bond", "indent", "pe"):
        assert np.array_equal(np.asarray(as_var[q]), np.asarray(as_num[q])), q
    assert not np.array_equal(as_num["x"], variable["x"])


# ------------------------------------------------------------------------------------------------------------------
# (c): the recorded minimisation
# ------------------------------------------------------------------------------------------------------------------
def test_minimisation(tmp_path, monkeypatch):
    """min_style cg on the globule inside a static sphere-in indenter with fix_modify energy yes: iterations, evaluations, stop
    index and list builds exactly; x and f under 16 x the recorded spread; every thermo column under 16 x its spread (at least
    the floor of reference_runs); and the wait budget of a minimisation, min_host_waits <= evals + rebuilds + iterations + 8."""
    set_env(monkeypatch, {})
    fx = ind.c_fixture()
    scn = fx.scn
    log = os.path.join(str(tmp_path), "log.indent")
    p = run_product(mn.script(scn), ind.c_system(), tmp_path, cmdargs=("-screen", "none", "-log", log))
    try:
        rows, st = mn.parse_log(open(log).read(), len(mn.columns(scn)))
        stat = {k: p.stat(k) for k in ("min_iterations", "min_evals", "min_stop", "min_host_waits", "min_rebuilds", "neigh_builds")}
        x, f, image = p.gather("x"), p.gather("f"), p.gather("image")
        sums = [p.extract_fix("c", 0, 0)] + [p.extract_fix("c", 0, 1, k) for k in range(3)]
    finally:
        p.close()
    want = fx.stats()
    assert (st["iterations"], st["evals"], st["stop"]) == (int(want["iterations"]), int(want["evals"]), int(want["stop"]))
    assert st["builds"] == list(fx.z["builds"]) and int(stat["neigh_builds"]) == int(fx.z["builds"][-1])
    assert np.array_equal(image, fx.z["image"])
    sp = fx.meta["spread"]
    dx, df = float(np.abs(x - fx.z["x"]).max()), float(np.abs(f - fx.z["f"]).max())
    print("minimisation: x %.2e (bound %.2e) f %.2e (bound %.2e)" % (dx, mn.FACTOR * sp["x"], df, mn.FACTOR * sp["f"]))
    assert dx <= mn.FACTOR * sp["x"] and df <= mn.FACTOR * sp["f"]
    assert rows.shape == fx.z["thermo"].shape
    bound = np.maximum(mn.FACTOR * np.asarray(sp["thermo"]), rr.THERMO_FLOOR * np.maximum(1.0, np.abs(fx.z["thermo"][:, 1:])))
    dev = np.abs(rows[:, 1:] - fx.z["thermo"][:, 1:])
    print("minimisation: thermo columns at most %.2e of their bounds" % float((dev / bound).max()))
    assert (dev <= bound).all(), (dev / bound).max()
    n = len(x)
    assert rel(np.array(sums) / n, fx.z["thermo"][-1][fx.col("f_c"):fx.col("f_c") + 4]) < 1e-9 and abs(sums[0]) > 0
    assert stat["min_host_waits"] <= stat["min_evals"] + stat["min_rebuilds"] + stat["min_iterations"] + 8, stat


# ------------------------------------------------------------------------------------------------------------------
# a restart in the middle of the ramp
# ------------------------------------------------------------------------------------------------------------------
def test_restart_mid_ramp(tmp_path, monkeypatch):
    """run 24, write_restart; a new handle: read_restart, the settings and fixes given again, the indenter with the ramp's
    remaining span, run 24 - bit for bit the engine's own continuation on the first handle, which is `unfix`, the same remaining
    ramp, run 24 (a single `run 48` evaluates ramp(a, b) where these evaluate ramp(mid, b): the radii agree to rounding, not to
    the bit - and a second `run` command repeats the set-up, which takes 3 N draws from fix langevin's stream, so the two halves
    are another trajectory than one `run 48`: x differs by 2e-2, v by 0.8 after 48 steps, measured).  (Restart files do not carry
    the fix.)  That the remaining ramp starts where the first half's ended is held without a device, in
    test_indent_cpu.py::test_vdisplace, through the table a step's launch carries."""
    from lammps_le_amd import lammps
    set_env(monkeypatch, PLAIN)
    fx = ind.fixture("shrink")
    a, b = ind.b_params()["shrink"]
    mid = a + 0.5 * (b - a)
    lines = fx.scn["script"].split("\n")
    head = lines[:ind.first_run_line(lines)]
    rest = ["variable R delete", "variable R equal ramp(%.17g,%.17g)" % (mid, b)] + [ln for ln in head if ln.startswith(("fix c ", "fix_modify c "))]
    rfile = os.path.join(str(tmp_path), "mid.restart")
    whole = run_product("\n".join(head + ["run 24", "write_restart " + rfile, "unfix c"] + rest + ["run 24"]), fx.system(), tmp_path)
    again = lammps(cmdargs=["-screen", "none"])
    try:
        again.command("read_restart " + rfile)
        for ln in head:
            w = ln.split()
            if w and w[0] not in ("units", "atom_style", "newton", "read_data", "variable") and not ln.startswith(("fix c ", "fix_modify c ")):
                again.command(ln)
        for ln in rest[1:]:
            again.command(ln)
        again.command("run 24")
        for q in ("x", "v", "f", "image", "type"):
            assert np.array_equal(whole.gather(q), again.gather(q)), q
        assert whole.extract_fix("c", 0, 0) == again.extract_fix("c", 0, 0) != 0.0
        assert int(again.stat("steps_fused_indent")) == 21 and int(whole.stat("steps_fused_indent")) == 21
    finally:
        whole.close()
        again.close()


def test_nothing_left_allocated(tmp_path, monkeypatch):
    """Nothing outlives the handle (the hook of test_gpu_devmem.py): the rows of block sums of k_indent and the empty wall table of
    a run with indenters alone belong to the handle's registry and go with close()."""
    from test_gpu_devmem import live
    set_env(monkeypatch, PLAIN)
    before = live()
    fx = ind.fixture("shrink")
    p = run_product(fx.scn["script"], fx.system(), tmp_path)
    assert int(p.stat("steps_fused_indent")) == 43 and p.stat("device_bytes") > 0
    p.close()
    assert live() == before
