"""The HIP path against recorded runs of the reference program (tests/golden/ref_*.npz; scenario table and comparison code:
reference_runs.py; the same fixtures hold the CPU oracle in test_reference_runs_cpu.py).  Nothing here reads the reference or
its binary.

Exact: bond and angle rows as multisets, per-atom bond counts, per-atom counts of the angles a bead is the centre of (the rest of
num_angle is not observable in the reference: see compare_end), types, image flags, the bonds / angles counts, the
fix vectors, the list builds of the last run.  Continuous: unwrapped x, v, f and the thermo rows under 16 x max(spread the
reference shows against itself from starts moved by one ulp, deviation of the oracle from the same fixture in this test run);
nothing is derived from the engine's output.  An FP32 intermediate in a force moves x by ~1e-9 within 64 steps; the bounds on
x are 2.0e-13 to 8.0e-13.

Measured on an MI355X, the largest over all tests of this file: the engine at 0.05 of its bound in x, 0.06 in v and f, 0.09 in a
thermo column; figures in the docstrings of the tests."""
import ctypes
import os

import numpy as np
import pytest

import reference_runs as rr
from systems import run_product

pytestmark = pytest.mark.gpu

PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
SHAPES = {"default": {}, "plain": PLAIN, "ahead": AHEAD, "unfused": {"LAMMPS_LE_NO_FUSE": "1"}}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_RNG_SEGMENTS", "LAMMPS_LE_RNG_W", "LAMMPS_LE_RNG_MODE",
            "LAMMPS_LE_RNG_B")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused")
CONTINUOUS = ("temp", "epair", "emol", "etotal", "press")
TENSOR = ("pxx", "pyy", "pzz", "pxy", "pxz", "pyz")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def engine_run(name, tmp_path, steps=None):
    """The engine after `steps` steps of the scenario (default: all), in the form reference_runs.oracle_run gives the oracle."""
    fx = rr.fixture(name)
    steps = fx.last if steps is None else steps
    # (the engine evaluates the pressure tensor only where a thermo_style line names it: the columns the reference recorded)
    lines = rr.script_for_steps(fx.scn, steps).split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run "))
    lines.insert(k, "thermo_style custom " + " ".join(("step",) + rr.THERMO))
    p = run_product("\n".join(lines), fx.system(), tmp_path)
    try:
        nb = p.gather("num_bond")
        got = dict(bond=rr.bond_rows(nb, p.gather("bond_type"), p.gather("bond_atom")), angle=None, type=p.gather("type"),
                   image=p.gather("image"), x=p.gather("x"), v=p.gather("v"), f=p.gather("f"), bonds=float(p.get_thermo("bonds")),
                   fixvec={fid: (float(p.extract_fix(fid, 0, 1, 0)), float(p.extract_fix(fid, 0, 1, 1))) for fid in fx.scn["fixes"]},
                   builds=int(p.stat("neigh_builds")), stats={k: int(p.stat(k)) for k in STATS}, num_bond=nb,
                   fene=int(p.stat("fene_warnings")))
        if rr.has_angles(fx.scn):
            na = p.gather("num_angle")
            got["angle"] = rr.angle_rows(na, p.gather("angle_type"), p.gather("angle_atom1"), p.gather("angle_atom2"), p.gather("angle_atom3"))
            got["angles"], got["num_angle"] = float(p.extract_setting("nangles")), na
            got["centre_slots"] = (p.gather("angle_atom2") == np.arange(1, len(na) + 1)[:, None]) & (np.arange(p.gather("angle_atom2").shape[1])[None, :] < na[:, None])
        got["rows"] = [dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5], bonds=r[6]) for r in p.thermo_history()]
        got["rows"][-1].update({k: p.get_thermo(k) for k in TENSOR})
    finally:
        p.close()
    return got


def compare_end(name, got, label):
    """Everything the fixture holds about the state after the last step."""
    fx, o = rr.fixture(name), rr.oracle_run(name)
    bad = rr.check_discrete(fx, fx.last, got)
    if got["builds"] != fx.z["builds"][-1]:
        bad.append("list builds of the last run: %d against %d recorded" % (got["builds"], fx.z["builds"][-1]))
    # per-atom counts: every bond is stored at both ends (newton_bond off); the reference has no per-atom output of its
    # angle counts (ex_load does not store a new angle at all three atoms) - the angle rows and the angles count stand for them
    ref = fx.rows_at(fx.last)
    if not np.array_equal(got["num_bond"], np.bincount(ref[:, 1:].reshape(-1) - 1, minlength=len(got["type"]))):
        bad.append("num_bond is not what the recorded rows give")
    if rr.has_angles(fx.scn) and "num_angle" in got:
        # num_angle: the reference writes no per-atom angle count, and its ex_load does not store a new angle at all three of
        # its atoms, so the count of a bead cannot be derived from the rows.  What the rows do fix: the number of angles a bead
        # stores as their CENTRE (the recorded rows are the centre copies) - exactly - and with it a lower limit of num_angle
        centre = np.bincount(fx.angles_at(fx.last)[:, 2] - 1, minlength=len(got["type"]))
        if not np.array_equal(got["centre_slots"].sum(axis=1), centre):
            bad.append("angles stored at their centre atom: per-atom counts differ from the recorded rows")
        if not (got["num_angle"] >= centre).all():
            bad.append("num_angle below the number of recorded angles around the bead")
    if got["fene"] != fx.meta["fene_warnings"]:
        bad.append("FENE warnings: %d against %d recorded" % (got["fene"], fx.meta["fene_warnings"]))
    odev = rr.deviation(fx, fx.last, o["x"], o["image"], o["v"], o["f"])
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), label, odev)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], CONTINUOUS + TENSOR), label,
                           rr.thermo_deviation(fx, o["rows"], CONTINUOUS + TENSOR))
    if [r["bonds"] for r in got["rows"]] != list(fx.thermo()[:, fx.col("bonds")]):
        bad.append("the bonds column differs from the recorded one")
    return bad


def thermo_steps(fx):
    """Steps of a one-run scenario after which thermo output comes: they take another path than the rest."""
    every = int(next(ln for ln in fx.scn["script"].split("\n") if ln.startswith("thermo ")).split()[1])
    return len([s for s in range(1, fx.last + 1) if s % every == 0 or s == fx.last])


def expected_paths(fx, shape):
    """step_plan.h at 1000 beads: the default is four lanes per bead (angles: one lane, loads ahead), whose thermo steps take the
    unfused kernels; only the throughput shape (plain) has an energy variant, and not with angles or fixes on a group."""
    t, s = thermo_steps(fx), fx.last
    grouped = "mobile" in fx.scn["script"]
    if shape == "unfused":
        return dict(steps_unfused=s)
    if shape == "plain" and not grouped and not rr.has_angles(fx.scn):
        return dict(steps_fused=s - t, steps_fused_thermo=t)
    return dict(steps_fused=s - t, steps_unfused=t, **(dict(steps_fused_group=s - t) if grouped else {}))


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.NAMES)
def test_engine_ends_where_the_reference_ends(tmp_path, monkeypatch, name):
    """Every scenario in the default shape, against the recorded end state.
    Measured on an MI355X (engine / oracle deviation from the fixture / recorded spread, the largest over the scenarios):
    x 1.4e-14 / 1.2e-14 / 5.0e-14 (smallest bound 2.0e-13), v 3.2e-13 / 3.0e-13 / 5.2e-13 (5.1e-12), f 2.2e-11 / 2.4e-11 / 4.0e-11
    (2.8e-10); thermo columns at most 0.09 of their bound.  The two respa scenarios are the ones that failed before fix
    extrusion was made idle under respa, as it is in the reference (oracle/AUDIT.md R1)."""
    set_env(monkeypatch, {})
    bad = compare_end(name, engine_run(name, tmp_path), name)
    assert not bad, "\n".join(bad)


FAMILIES = ["cycle_tp05", "sort3", "group_anchored", "angle_harmonic"]


@pytest.mark.parametrize("shape", ["plain", "ahead", "unfused"])
@pytest.mark.parametrize("name", FAMILIES)
def test_shapes_of_the_step_kernel(tmp_path, monkeypatch, name, shape):
    """The LE cycle, the sorted cycle, the fixes on a group and the angle scenario in the other shapes of the step kernel (one
    lane per bead without and with loads issued ahead, and the unfused kernels), with the path the steps took: the same end
    state under the same bounds.  Measured on an MI355X: within the figures of the default shape (x 1.4e-14, v 3.2e-13, f 2.2e-11)."""
    set_env(monkeypatch, SHAPES[shape])
    got = engine_run(name, tmp_path)
    bad = compare_end(name, got, "%s %s" % (name, shape))
    assert not bad, "\n".join(bad)
    assert got["stats"] == dict(dict.fromkeys(STATS, 0), **expected_paths(rr.fixture(name), shape)), got["stats"]


@pytest.mark.parametrize("name", FAMILIES)
def test_default_shape_takes_the_step_kernel(tmp_path, monkeypatch, name):
    set_env(monkeypatch, {})
    fx = rr.fixture(name)
    got = engine_run(name, tmp_path)
    assert got["stats"] == dict(dict.fromkeys(STATS, 0), **expected_paths(fx, "default")), got["stats"]


@pytest.mark.parametrize("name", [s["name"] for s in rr.SCENARIOS if len(s["checkpoints"]) > 1])
def test_earlier_checkpoint(tmp_path, monkeypatch, name):
    """One scenario per fix family (LE cycle, sorted, stock, group, langevin keywords, respa, angles): a fresh run up to the
    earlier recorded checkpoint - rows, types, image flags exactly, x and v under 16 x max(spread, oracle deviation) there.
    Measured on an MI355X: x at most 5.3e-15 (oracle 3.6e-15, spread 1.8e-14, smallest bound 1.4e-13), v 2.8e-13 (1.1e-13,
    5.4e-13, 4.4e-12)."""
    set_env(monkeypatch, {})
    fx = rr.fixture(name)
    step = fx.checkpoints[0]
    got, o = engine_run(name, tmp_path, step), rr.oracle_run(name, step)
    bad = rr.check_discrete(fx, step, got)
    bad += rr.check_continuous(fx, step, rr.deviation(fx, step, got["x"], got["image"], got["v"]), name,
                               rr.deviation(fx, step, o["x"], o["image"], o["v"]))
    assert not bad, "\n".join(bad)


def test_langevin_pools_switch_inside_the_run(tmp_path, monkeypatch):
    """The Langevin keyword scenario with draw pools of three steps (LAMMPS_LE_RNG_W=3): some twenty pool switches inside the
    64 steps, the same recorded end state."""
    set_env(monkeypatch, {"LAMMPS_LE_RNG_W": "3"})
    bad = compare_end("langevin_scale_zero", engine_run("langevin_scale_zero", tmp_path), "langevin W=3")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the draws
# ------------------------------------------------------------------------------------------------------------------
def recorded_draws(seed):
    with np.load(os.path.join(rr.GOLDEN, "ref_ranmars.npz")) as z:
        return z["seed_%d" % seed].astype(np.int64)


RNG = {"default": {}, "segments3": {"LAMMPS_LE_RNG_SEGMENTS": "3"}, "segments7": {"LAMMPS_LE_RNG_SEGMENTS": "7"},
       "w3": {"LAMMPS_LE_RNG_W": "3"}, "block": {"LAMMPS_LE_RNG_MODE": "block"}}


@pytest.mark.parametrize("variant", sorted(RNG))
def test_langevin_draws_are_the_recorded_ones(tmp_path, monkeypatch, variant):
    """1112 beads at rest, three `run 0`: the forces are the Langevin draws alone, and as 24-bit integers they are the 10008
    the reference drew, for the six seeds - with the batch generator, cut into 3 and 7 segments, with pools of three steps
    and with the block generator."""
    set_env(monkeypatch, RNG[variant])
    s = rr.ranmars_system()
    for seed in rr.RANMARS_SEEDS:
        p = run_product(rr.ranmars_script(seed), s, tmp_path)
        f = []
        for _ in range(rr.RANMARS_RUNS):
            p.command("run 0")
            f.append(p.gather("f"))
        p.close()
        got, off = rr.draws_from_forces(np.concatenate(f))
        assert off < 1e-8, off
        assert np.array_equal(got, recorded_draws(seed)), (variant, seed, np.nonzero(got != recorded_draws(seed))[0][:5])


def test_device_generator_gives_the_recorded_stream(monkeypatch):
    set_env(monkeypatch, {})
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_device_ranmars
    fn.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    for seed in rr.RANMARS_SEEDS:
        want = recorded_draws(seed)
        for skip in (0, 1, 97, 5000):
            for ncalls in (1, 3, 7):
                count = len(want) - skip
                out = np.zeros(count)
                assert fn(seed, skip, count, ncalls, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
                assert np.array_equal(out * 16777216.0, want[skip:]), (seed, skip, ncalls)


# ------------------------------------------------------------------------------------------------------------------
# decomposed: z slabs on 2 and 3 ranks (threads of this process, in-process transport)
# ------------------------------------------------------------------------------------------------------------------
def rank_results(lmp):          # (every rank calls it)
    return dict(f=lmp.gather("f"), type=lmp.gather("type"), rows=lmp.thermo_history(), bonds=lmp.get_thermo("bonds"),
                fene=lmp.stat("fene_warnings"), ranks=lmp.stat("comm_nranks"), nlocal=lmp.stat("nlocal"))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["slabs_cycle", "slabs_sort"])
def test_decomposed(tmp_path, monkeypatch, name, world):
    """The barrier cycle and the sorted one on 2048 beads, cut into 2 and 3 slabs along z (ghost cutoff 3.3, the widest both
    slab counts admit in that box; extruder bonds cross the faces between the slabs and stay below 3.0: the scenario's own
    condition), through test_gpu_dd.run_ranks_local: the joined state against the same recorded one-rank run of the reference
    under the same comparison as on one GPU (without the pressure tensor, which a decomposed run does not hand out)."""
    from test_gpu_dd import run_ranks_local
    set_env(monkeypatch, {})
    fx = rr.fixture(name)
    r = run_ranks_local(world, fx.system(), fx.scn["script"], tmp_path, extra=rank_results)
    assert r["ranks"] == world and 0 < r["nlocal"] < fx.scn["system"]["n"]
    got = dict(bond=rr.bond_rows(r["num_bond"], r["bond_type"], r["bond_atom"]), angle=None, type=r["type"], image=r["image"],
               x=r["x"], v=r["v"], f=r["f"], bonds=float(r["bonds"]), num_bond=r["num_bond"], fene=int(r["fene"]),
               fixvec={fid: (float(r["f_" + fid][0]), float(r["f_" + fid][1])) for fid in fx.scn["fixes"]}, builds=int(r["builds"][0]),
               rows=[dict(step=int(q[0]), temp=q[1], epair=q[2], emol=q[3], etotal=q[4], press=q[5], bonds=q[6]) for q in r["rows"]])
    bad = compare_end(name, got, "%s on %d slabs" % (name, world))
    assert not bad, "\n".join(bad)
