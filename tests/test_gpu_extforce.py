"""fix spring/self, fix addforce and fix setforce on the HIP path: k_fixforce and the EXT variant of the step kernel against
recorded runs of the reference binary (tests/golden/extforce_*.npz, scenario table extforce_runs.py) and against the long-double
restatement (extforce_reference.py).  Nothing here reads the reference or its binary.

`run 0`: the engine's forces with the four fixes against extforce_reference applied to the engine's own forces without them, the
fixes' sums and their share of pe and press likewise.  The bounds are 16 x the two figures the generator wrote into
extforce_runs.json for the reference binary's own operation order against the same restatement - 16 is reference_runs.FACTOR,
the factor the wall tests hold their recorded runs to.  The 48-step runs: bond rows, counters and list builds exactly, x / v / f
under 16 x the spread the reference shows against itself from starts moved by one ulp, thermo columns within the bounds
reference_runs derives from the same spread - in the three shapes of the step kernel and through the unfused kernels, with the
path the steps took."""
import os

import numpy as np
import pytest

import extforce_runs as ex
import reference_runs as rr
from systems import run_product

pytestmark = pytest.mark.gpu

FACTOR = rr.FACTOR
PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD, "unfused": {"LAMMPS_LE_NO_FUSE": "1"}}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall", "steps_fused_soft", "steps_fused_ext")
CONTINUOUS = ("temp", "epair", "emol", "etotal", "press")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ------------------------------------------------------------------------------------------------------------------
# run 0: k_fixforce<EFLAG>, the column sums, eval_thermo
# ------------------------------------------------------------------------------------------------------------------
def test_run0(tmp_path, monkeypatch):
    """Two tethers, an addforce and a setforce on overlapping groups, members with image flags of +-1 and +-2."""
    set_env(monkeypatch, {})
    s, m = ex.a_system(), ex.meta()["a"]
    n = len(s["x"])
    first, second = ex.a_script().split("unfix s\n")
    p = run_product(first, s, tmp_path)
    f = p.gather("f")
    assert np.array_equal(p.gather("x"), ex.a_positions()) and np.array_equal(p.gather("image"), s["image"])
    sums = [p.extract_fix("s", 0, 0), p.extract_fix("s2", 0, 0), p.extract_fix("a", 0, 0)] + \
           [p.extract_fix("a", 0, 1, k) for k in range(3)] + [p.extract_fix("z", 0, 1, k) for k in range(3)]
    pe, press = p.get_thermo("pe"), p.get_thermo("press")
    assert int(p.stat("steps_fused")) == 0
    for ln in ("unfix s\n" + second).split("\n"):
        p.command(ln)
    f0 = p.gather("f")
    pe0, press0 = p.get_thermo("pe"), p.get_thermo("press")
    p.close()
    fx = ex.a_fixture()
    ref_f, cols, ref_pe, ref_press = ex.a_reference(f0)
    k = ex.A_THERMO.index("f_s")
    figures = {
        "f against extforce_reference on the engine's own f0": (rel(ref_f, f), m["reference_operation_order"]),
        "the fixes' sums against extforce_reference": (rel(cols, np.array(sums) / n), m["reference_sums"]),
        "share of pe": (rel(ref_pe, pe - pe0), m["reference_sums"]),
        "share of press": (rel(ref_press, press - press0), m["reference_sums"]),
    }
    # for the record, not asserted (the engine's pair and bond forces are not the reference binary's to the last bit, and
    # setforce's foriginal sums carry them): the distance to the recorded run itself
    print("f against the recorded run: %.2e; f0: %.2e; the fixes' columns against the recorded row: %.2e" %
          (rel(f, fx["f"]), rel(f0, fx["f0"]), rel(np.array(sums) / n, fx["row"][k:])))
    bad = []
    for what, (err, figure) in figures.items():
        print("%-56s %.2e  recorded figure %.2e  bound %.2e" % (what, err, figure, FACTOR * figure))
        if not err <= FACTOR * figure:
            bad.append("%s: %.3e exceeds %.3e" % (what, err, FACTOR * figure))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the 48-step recorded runs
# ------------------------------------------------------------------------------------------------------------------
def engine_run(name, tmp_path, script=None):
    fx = ex.fixture(name)
    lines = (script or fx.scn["script"]).split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("run_style"))
    lines.insert(k, "thermo_style custom " + " ".join(("step",) + rr.THERMO))
    p = run_product("\n".join(lines), fx.system(), tmp_path)
    try:
        nb = p.gather("num_bond")
        got = dict(bond=rr.bond_rows(nb, p.gather("bond_type"), p.gather("bond_atom")), angle=None, type=p.gather("type"),
                   image=p.gather("image"), x=p.gather("x"), v=p.gather("v"), f=p.gather("f"), bonds=float(p.get_thermo("bonds")),
                   fixvec={fid: (float(p.extract_fix(fid, 0, 1, 0)), float(p.extract_fix(fid, 0, 1, 1))) for fid in fx.scn["fixes"]},
                   builds=int(p.stat("neigh_builds")), stats={k: int(p.stat(k)) for k in STATS}, fene=int(p.stat("fene_warnings")),
                   pe=p.get_thermo("pe"))
        got["ext"] = {}
        for nm in fx.scn["ext_columns"]:
            if nm == "pe":
                continue
            fid, _, idx = nm[2:].partition("[")
            got["ext"][nm] = p.extract_fix(fid, 0, 1, int(idx[:-1]) - 1) if idx else p.extract_fix(fid, 0, 0)
        got["rows"] = [dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5], bonds=r[6]) for r in p.thermo_history()]
    finally:
        p.close()
    return got


def compare_end(name, got, label):
    fx = ex.fixture(name)
    bad = rr.check_discrete(fx, fx.last, got)
    if got["builds"] != fx.z["builds"][-1]:
        bad.append("list builds of the last run: %d against %d recorded" % (got["builds"], fx.z["builds"][-1]))
    if got["fene"] != fx.meta["fene_warnings"]:
        bad.append("FENE warnings: %d against %d recorded" % (got["fene"], fx.meta["fene_warnings"]))
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), label)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], CONTINUOUS), label)
    if [r["bonds"] for r in got["rows"]] != list(fx.thermo()[:, fx.col("bonds")]):
        bad.append("the bonds column differs from the recorded one")
    if fx.scn["ext_columns"]:
        # the last row: pe with the fixes' energies in it, and the fixes' columns (recorded per atom: thermo_modify norm yes)
        n, row, last = len(got["type"]), fx.thermo()[-1], len(fx.thermo()) - 1
        dev = {}
        for nm in fx.scn["ext_columns"]:
            dev[(last, nm)] = abs((got["pe"] if nm == "pe" else got["ext"][nm] / n) - row[fx.col(nm)])
        bad += rr.check_thermo(fx, dev, label)
    return bad


def expected_paths(name, shape):
    """48 steps with `thermo 10`: five thermo steps (10 .. 40 and 48), which a run with these fixes takes through the unfused
    kernels in every shape; r-RESPA is unfused altogether.  tether_between: the last run is its second, 24 steps with the
    tether - thermo steps 30, 40, 48."""
    zero = dict.fromkeys(STATS, 0)
    if name == "tether_between":
        return dict(zero, steps_unfused=24) if shape == "unfused" else dict(zero, steps_fused=21, steps_fused_ext=21, steps_unfused=3)
    if shape == "unfused" or name == "respa2":
        return dict(zero, steps_unfused=48)
    if name == "add_every3":
        # steps 9, 18 and 39 as well: the last on which the addforce acts before a thermo step it skips (10, 20, 40) - its sums
        # of that step are what the thermo row shows, as in the reference
        return dict(zero, steps_fused=40, steps_fused_ext=40, steps_unfused=8)
    return dict(zero, steps_fused=43, steps_fused_ext=43, steps_unfused=5)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ex.NAMES)
def test_recorded_runs(tmp_path, monkeypatch, name, shape):
    """Every recorded run in the three shapes of the step kernel and through the unfused kernels; the plain steps of a fused
    shape go through k_step<..., EXT> (steps_fused_ext), the thermo steps do not."""
    set_env(monkeypatch, SHAPES[shape])
    got = engine_run(name, tmp_path)
    bad = compare_end(name, got, "%s %s" % (name, shape))
    assert not bad, "\n".join(bad)
    assert got["stats"] == expected_paths(name, shape), got["stats"]


_WITH_COLUMNS = [s["name"] for s in ex.SCENARIOS if s["ext_columns"]]


@pytest.mark.parametrize("step", [10, 20, 30, 40])
@pytest.mark.parametrize("name", _WITH_COLUMNS)
def test_fix_columns_of_every_row(tmp_path, monkeypatch, name, step):
    """The fixes' own columns and pe at the thermo rows inside the run (the engine's thermo history keeps the seven standard
    columns, so test_recorded_runs reaches the fixes' columns on the last row alone): the scenario cut to `step` steps - a run
    that long ends in the state of that step of the full run, reference_runs.script_for_steps - and f_ID, f_ID[k] through
    extract_fix against the recorded row, under the same bounds.  add_every3: rows 10, 20 and 40 are thermo steps the addforce
    skips; it reports the sums of steps 9, 18 and 39 there."""
    set_env(monkeypatch, PLAIN)
    fx = ex.fixture(name)
    got = engine_run(name, tmp_path, script=rr.script_for_steps(fx.scn, step))
    k = [i for i, r in enumerate(fx.thermo()) if int(r[0]) == step][-1]
    n, row = len(got["type"]), fx.thermo()[k]
    dev = {(k, nm): abs((got["pe"] if nm == "pe" else got["ext"][nm] / n) - row[fx.col(nm)]) for nm in fx.scn["ext_columns"]}
    bad = rr.check_thermo(fx, dev, "%s step %d" % (name, step))
    assert not bad, "\n".join(bad)
    if name != "respa2":
        assert got["stats"]["steps_fused_ext"] > 0


def test_skipped_setup_step_keeps_the_sums(tmp_path, monkeypatch):
    """An addforce with `every 3` after `run 4` (it acted at step 3), then a second run whose setup step 4 it skips: f_ID and
    f_ID[k] are still those of step 3, as the reference keeps foriginal over a run command; a new fix starts from zero."""
    set_env(monkeypatch, PLAIN)
    s = ex.a_system()
    from systems import CHAIN_SCRIPT
    p = run_product(CHAIN_SCRIPT + "fix 1 all nve\ngroup pull id 3:400:25\nfix a pull addforce 0.7 -1.3 2.1 every 3\nthermo 100\nrun 4\n", s, tmp_path)
    first = [p.extract_fix("a", 0, 0)] + [p.extract_fix("a", 0, 1, k) for k in range(3)]
    p.command("run 1")
    second = [p.extract_fix("a", 0, 0)] + [p.extract_fix("a", 0, 1, k) for k in range(3)]
    p.command("unfix a")
    p.command("fix a pull addforce 0.7 -1.3 2.0 every 3")
    p.command("run 0")          # step 5: the new fix has not acted yet
    third = [p.extract_fix("a", 0, 0)] + [p.extract_fix("a", 0, 1, k) for k in range(3)]
    p.close()
    assert all(v != 0.0 for v in first) and second == first and third == [0.0] * 4


@pytest.mark.parametrize("shape", ["plain", "ahead"])
def test_crossing_without_the_fused_binning(tmp_path, monkeypatch, shape):
    """The crossing with k_wrap_bin instead of the binning inside the step kernel (LAMMPS_LE_NO_FUSED_BIN): the image words
    are then written by another kernel at another place of the rebuild; pos + img * prd is the same unwrapped position."""
    set_env(monkeypatch, dict(SHAPES[shape], LAMMPS_LE_NO_FUSED_BIN="1"))
    got = engine_run("crossing", tmp_path)
    bad = compare_end("crossing", got, "crossing %s no fused bin" % shape)
    assert not bad, "\n".join(bad)
    assert got["stats"] == expected_paths("crossing", shape), got["stats"]


def test_first_run_before_the_tether_has_no_ext_steps(tmp_path, monkeypatch):
    """tether_between: the first run of the two has none of the fixes - its plain steps are the default instantiation's."""
    set_env(monkeypatch, PLAIN)
    fx = ex.fixture("tether_between")
    script = fx.scn["script"].split("fix s teth")[0]
    p = run_product(script, fx.system(), tmp_path)
    stats = {k: int(p.stat(k)) for k in STATS}
    p.close()
    assert stats["steps_fused_ext"] == 0 and stats["steps_fused"] == 21 and stats["steps_fused_thermo"] + stats["steps_unfused"] == 3, stats


# ------------------------------------------------------------------------------------------------------------------
# the engine against itself, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def _state(p):
    return {q: p.gather(q) for q in ("x", "v", "image", "type", "num_bond", "bond_atom")}


def _same(a, b):
    return [q for q in a if not np.array_equal(a[q], b[q])]


_SETTINGS = ("neighbor", "neigh_modify", "comm_modify", "bond_style", "bond_coeff", "pair_style", "pair_modify", "pair_coeff", "timestep",
             "special_bonds", "atom_modify")


def _after_restart(script):
    """The lines of a scenario script a handle needs after read_restart: the settings a restart file does not carry, the
    groups' fixes and everything behind them - without the lines that read the data file."""
    return [ln for ln in script.split("\n") if ln.split()[:1] and ln.split()[0] not in ("units", "atom_style", "newton", "read_data", "group")]


def test_restart_continues_bit_for_bit(tmp_path, monkeypatch):
    """run 24; write_restart; then a new handle: read_restart, the same fixes, run 24 - equals run 24; run 24 on one handle.
    The origins come from the file, not from the positions at the second fix command."""
    from lammps_le_amd import lammps
    set_env(monkeypatch, PLAIN)
    fx = ex.fixture("add_every3")
    head = fx.scn["script"].split("run %d" % ex.B_STEPS)[0]
    path = os.path.join(str(tmp_path), "mid.restart")
    a = run_product(head + "run 24\nwrite_restart %s\nrun 24\n" % path, fx.system(), tmp_path)
    want = _state(a)
    a.close()
    b = lammps(cmdargs=["-screen", "none"])
    b.command("read_restart " + path)
    for ln in _after_restart(head):
        b.command(ln)
    b.command("run 24")
    got = _state(b)
    assert int(b.stat("steps_fused_ext")) > 0
    b.close()
    assert _same(want, got) == []


def test_unfix_and_group_change_between_runs(tmp_path, monkeypatch):
    """`unfix` of the tether, and the tether given again on another group, between runs: each continuation equals a fresh
    handle started from a restart file written at that point (the method of test_fixes_change_their_group_between_runs)."""
    from lammps_le_amd import lammps
    set_env(monkeypatch, PLAIN)
    fx = ex.fixture("tether_behind")
    head = fx.scn["script"].split("run %d" % ex.B_STEPS)[0]
    r1, r2 = os.path.join(str(tmp_path), "one.restart"), os.path.join(str(tmp_path), "two.restart")
    a = run_product(head + "run 16\nwrite_restart %s\nunfix s\nrun 16\n" % r1, fx.system(), tmp_path)
    after_unfix = _state(a)
    assert int(a.stat("steps_fused_ext")) == 0 and int(a.stat("steps_fused")) > 0      # (no fix of the three is left)
    for ln in ("write_restart " + r2, "fix s pull spring/self 4.0", "run 16"):
        a.command(ln)
    want = _state(a)
    assert int(a.stat("steps_fused_ext")) > 0
    a.close()
    settings = [ln for ln in _after_restart(head) if ln.split()[0] in _SETTINGS or ln.split()[0] in ("thermo",)]
    fixes = [ln for ln in _after_restart(head) if ln.split()[0] == "fix" and ln.split()[1] != "s"]
    b = lammps(cmdargs=["-screen", "none"])
    b.command("read_restart " + r1)
    for ln in settings + fixes:
        b.command(ln)
    b.command("run 16")
    got_unfix = _state(b)
    b.close()
    assert _same(after_unfix, got_unfix) == []
    c = lammps(cmdargs=["-screen", "none"])
    c.command("read_restart " + r2)
    for ln in settings + fixes + ["fix s pull spring/self 4.0"]:
        c.command(ln)
    c.command("run 16")
    got = _state(c)
    c.close()
    assert _same(want, got) == []
