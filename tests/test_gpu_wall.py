"""fix wall/region on the HIP path: k_wall and the wall variant of the step kernel against recorded runs of the reference
binary (tests/golden/wall_*.npz, scenario table wall_runs.py) and against the long-double wall reference (wall_reference.py).
Nothing here reads the reference or its binary.

`run 0`: forces, f_ID, f_ID[k], pe and press of the five styles on every region, bound 1e-12 relative to max(1, |value|) (the
project's bound for single evaluations).  The LE cycle inside the WCA sphere, 48 steps: bond rows, counters and list builds
exactly, x / v / f under 16 x the spread the reference shows against itself from starts moved by one ulp, thermo columns
within the bounds reference_runs derives from the same spread - in the three shapes of the step kernel and through the
unfused kernels, with the path the steps took."""
import numpy as np
import pytest

import reference_runs as rr
import wall_reference as wr
import wall_runs as wl
from systems import CHAIN_SCRIPT, run_product

pytestmark = pytest.mark.gpu

RUN0_BOUND = 1e-12
PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD, "unfused": {"LAMMPS_LE_NO_FUSE": "1"}}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall")
CONTINUOUS = ("temp", "epair", "emol", "etotal", "press")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ------------------------------------------------------------------------------------------------------------------
# run 0: k_wall<EFLAG>, the column sums, eval_thermo
# ------------------------------------------------------------------------------------------------------------------
_f0 = {}


def forces_without_wall(tmp_path):
    if "f" not in _f0:
        p = run_product(wl.a_script(None, None, wall=False), wl.a_system(), tmp_path)
        _f0["f"] = p.gather("f")
        p.close()
    return _f0["f"]


@pytest.mark.parametrize("region", list(wl.REGIONS))
def test_run0(tmp_path, monkeypatch, region):
    """The five styles on one region: per-bead forces against the recorded ones, the wall's share of them (forces with minus
    forces without the wall, both the engine's) against wall_reference, f_ID and f_ID[1..3] (extract_fix: the sums; the thermo
    keyword: per atom under norm yes) against both, pe and press of the two `run 0` - fix_modify energy / virial no, then yes -
    against the recorded rows."""
    set_env(monkeypatch, {})
    fx, s = wl.a_fixture(region), wl.a_system()
    n = len(s["x"])
    f0 = forces_without_wall(tmp_path)
    reg = wr.parse_region(wl.REGIONS[region].split())
    bad = []
    for style in wl.STYLES:
        t = wr.wall_terms(s["x"], reg, wr.parse_wall(wl.STYLES[style].split()))
        lines = wl.a_script(region, style).split("\n")
        cut = lines.index("fix_modify w energy yes virial yes")
        p = run_product("\n".join(lines[:cut]), s, tmp_path)
        rows = fx["rows_" + style]
        col = wl.A_THERMO.index
        f = p.gather("f")
        figures = {"f against the recorded run": rel(f, fx["f_" + style]),
                   "wall share against wall_reference": float((np.abs((f - f0) - t["f"].astype(np.float64)) / np.maximum(1.0, np.abs(f))).max())}
        for run in (0, 1):
            if run:
                p.command("fix_modify w energy yes virial yes")
                p.command("run 0")
            sums = [p.extract_fix("w", 0, 0)] + [p.extract_fix("w", 0, 1, k) for k in range(3)]
            figures["run %d f_ID sums against wall_reference" % run] = rel(sums, [float(t["energy"])] + [float(v) for v in t["fwall"]])
            figures["run %d f_ID sums against the recorded rows" % run] = rel(np.array(sums) / n, rows[run][col("f_w"):col("f_w") + 4])
            figures["run %d pe" % run] = rel(p.get_thermo("pe"), rows[run][col("pe")])
            figures["run %d press" % run] = rel(p.get_thermo("press"), rows[run][col("press")])
        assert int(p.stat("steps_fused")) == 0
        p.close()
        for what, err in figures.items():
            print("%-14s %-9s %-46s %.2e" % (region, style, what, err))
            if not err < RUN0_BOUND:
                bad.append("%s %s %s: %.3e exceeds %.1e" % (region, style, what, err, RUN0_BOUND))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the LE cycle inside the sphere: the recorded runs
# ------------------------------------------------------------------------------------------------------------------
def engine_run(name, tmp_path):
    fx = wl.fixture(name)
    lines = fx.scn["script"].split("\n")
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
        if fx.scn["wall_columns"]:
            got["wall"] = [p.extract_fix("w", 0, 0)] + [p.extract_fix("w", 0, 1, k) for k in range(3)]
        got["rows"] = [dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5], bonds=r[6]) for r in p.thermo_history()]
    finally:
        p.close()
    return got


def compare_end(name, got, label):
    fx = wl.fixture(name)
    bad = rr.check_discrete(fx, fx.last, got)
    if got["builds"] != fx.z["builds"][-1]:
        bad.append("list builds of the last run: %d against %d recorded" % (got["builds"], fx.z["builds"][-1]))
    if got["fene"] != fx.meta["fene_warnings"]:
        bad.append("FENE warnings: %d against %d recorded" % (got["fene"], fx.meta["fene_warnings"]))
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), label)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], CONTINUOUS), label)
    if [r["bonds"] for r in got["rows"]] != list(fx.thermo()[:, fx.col("bonds")]):
        bad.append("the bonds column differs from the recorded one")
    if fx.scn["wall_columns"]:
        # the last row: pe with the wall's energy in it, f_w and f_w[1..3] (recorded per atom: thermo_modify norm yes)
        n, row = len(got["type"]), fx.thermo()[-1]
        dev = {(len(fx.thermo()) - 1, "pe"): abs(got["pe"] - row[fx.col("pe")])}
        for k, nm in enumerate(wl.WALL_COLUMNS[1:]):
            dev[(len(fx.thermo()) - 1, nm)] = abs(got["wall"][k] / n - row[fx.col(nm)])
        bad += rr.check_thermo(fx, dev, label)
    return bad


def expected_paths(name, shape):
    """48 steps with `thermo 10`: five thermo steps, which a run with walls takes through the unfused kernels in every shape;
    r-RESPA and a wall on a group are unfused altogether; after the unfix the second run (24 steps, three thermo steps) has no
    wall: the throughput shape takes its thermo steps through the energy variant."""
    zero = dict.fromkeys(STATS, 0)
    if name == "unfix_between":
        if shape == "unfused":
            return dict(zero, steps_unfused=24)
        return dict(zero, steps_fused=21, **({"steps_fused_thermo": 3} if shape == "plain" else {"steps_unfused": 3}))
    if shape == "unfused" or name in ("respa2", "group"):
        return dict(zero, steps_unfused=48)
    return dict(zero, steps_fused=43, steps_fused_wall=43, steps_unfused=5)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", wl.NAMES)
def test_recorded_runs(tmp_path, monkeypatch, name, shape):
    """Every recorded run in the three shapes of the step kernel and through the unfused kernels.  Measured on an MI355X, the
    largest over the 24 cases: x 8.9e-15 (smallest bound 2.3e-13), v 1.7e-13 (4.8e-12), f 1.5e-11 (2.8e-10); thermo columns,
    pe and f_w[k] at most a tenth of their bounds.  `run 0` (test_run0): at most 9.2e-14 (sphere_out morse, forces against the
    recorded run) against 1e-12."""
    set_env(monkeypatch, SHAPES[shape])
    got = engine_run(name, tmp_path)
    bad = compare_end(name, got, "%s %s" % (name, shape))
    assert not bad, "\n".join(bad)
    assert got["stats"] == expected_paths(name, shape), got["stats"]


def test_first_run_before_the_unfix_is_fused(tmp_path, monkeypatch):
    """(c): the first run of the two, with the wall: 24 steps, thermo steps 10, 20, 24."""
    set_env(monkeypatch, PLAIN)
    fx = wl.fixture("unfix_between")
    script = fx.scn["script"].split("unfix w")[0]
    p = run_product(script, fx.system(), tmp_path)
    stats = {k: int(p.stat(k)) for k in STATS}
    p.close()
    assert stats == dict(dict.fromkeys(STATS, 0), steps_fused=21, steps_fused_wall=21, steps_unfused=3), stats


@pytest.mark.parametrize("name", ["langevin_then_wall", "wall_then_langevin"])
@pytest.mark.parametrize("shape", ["four", "plain", "ahead"])
def test_fused_against_unfused(tmp_path, monkeypatch, name, shape):
    """The same script through the wall variant of the step kernel and through k_wall: x to 1e-9, v to 1e-8 relative (what
    test_step_kernel_variants asks of the shapes), the same list builds and bond rows."""
    runs = {}
    for label, env in (("fused", SHAPES[shape]), ("unfused", SHAPES["unfused"])):
        set_env(monkeypatch, env)
        runs[label] = engine_run(name, tmp_path)
    a, b = runs["fused"], runs["unfused"]
    assert a["stats"]["steps_fused_wall"] == 43 and b["stats"]["steps_fused_wall"] == 0
    print("%s %s: x %.2e v %.2e" % (name, shape, rel(a["x"], b["x"]), rel(a["v"], b["v"])))
    assert rel(a["x"], b["x"]) < 1e-9 and rel(a["v"], b["v"]) < 1e-8
    assert a["builds"] == b["builds"] and np.array_equal(a["bond"], b["bond"]) and np.array_equal(a["image"], b["image"])


# ------------------------------------------------------------------------------------------------------------------
# a bead outside the region: an ordinary error through the flag word
# ------------------------------------------------------------------------------------------------------------------
def test_particle_outside(tmp_path, monkeypatch):
    from lammps_le_amd import LammpsError
    set_env(monkeypatch, {})
    s = wl.a_system()
    c = 0.5 * float(s["box"][0][1])
    far = float(np.sqrt(((s["x"] - c) ** 2).sum(axis=1)).max())
    base = CHAIN_SCRIPT + "fix 1 all nve\n"
    text = "Particle outside surface of region used in fix wall/region"
    # at run 0: the corner beads are outside a ball of radius 5
    p = run_product(base + "region ball sphere %g %g %g 5.0 side in\nfix w all wall/region ball harmonic 1.0 0.0 1.0\n" % (c, c, c), s, tmp_path)
    with pytest.raises(LammpsError, match=text):
        p.command("run 0")
    p.close()
    # inside a fused run: a wall without force (epsilon 0) 0.01 beyond the farthest bead, which thermal motion crosses
    p = run_product(base + "region ball sphere %.17g %.17g %.17g %.17g side in\nfix w all wall/region ball harmonic 0.0 0.0 0.5\n"
                    "thermo 1000\n" % (c, c, c, far + 0.01), s, tmp_path)
    p.command("run 0")
    with pytest.raises(LammpsError, match=text):
        p.command("run 400")
    assert int(p.stat("steps_fused_wall")) > 0
    p.close()
    # and the device is as it was: another handle runs
    p = run_product(base + "region ball sphere %g %g %g 9.0 side in\nfix w all wall/region ball lj126 1.0 1.0 1.1\nrun 5\n" % (c, c, c), s, tmp_path)
    assert int(p.stat("steps_fused_wall")) == 4
    p.close()
