"""fix wall/region on the HIP path, step by step: the wall variant of the step kernel against the long-double velocity Verlet
of force_reference.py with the wall term of wall_reference.py added; a wall on a group beside beads it must not touch; walls
in decomposed runs.

Twelve steps: the input `offset` of force_inputs.py (630 beads, temperature 5, neighbor 0.2: three or four list builds) around
a small ball (`sphere ... side out`) that sits in the largest hole of the start; its lj126 wall reaches the beads within 2.29
of the centre.  The ball and its cutoff lie 0.2 inside every box face (a stored coordinate leaves the box by at most half
the skin, 0.1), so the wall never sees a coordinate that is waiting for
its wrap.  fix_modify energy yes virial yes: etotal and press of every thermo row carry the wall's energy and virial.  Bounds:
those of test_gpu_force.py for the same comparison without the wall - 16 x the deviation of the FP64 oracle from the reference
on the same input and fixes (the oracle has no wall), at least 1e-13, never above 1e-9 (x, rows) and 1e-8 (v, f)."""
import functools
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import force_compare as fc
import force_inputs as fi
import force_reference as fr
import reference_runs as rr
import wall_reference as wr
import wall_runs as wl
from systems import CHAIN_SCRIPT, lattice_chain, run_product, wrap_into_box

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


# ------------------------------------------------------------------------------------------------------------------
# twelve steps against force_reference's velocity Verlet with the wall term added
# ------------------------------------------------------------------------------------------------------------------
NAME = "offset"
BALL_RADIUS = 0.05
WALL = dict(style="lj126", epsilon=1e-5, sigma=2.0, cutoff=2.24)           # (its minimum is at 2.2449: repulsive throughout)
MARGIN = 0.2
THERMO = 4
# the fixes of a case: force_compare.FIXES' name (model, oracle deviations) and the lines, with %s for the wall
ORDERS = {
    "nve": ("nve", "fix 1 all nve\n%s"),
    "wall-langevin": ("langevin", "fix 1 all nve\n%sfix 2 all langevin 1.0 1.0 1.0 " + str(fc.LANGEVIN_SEED) + "\n"),
    "langevin-wall": ("langevin", "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 " + str(fc.LANGEVIN_SEED) + "\n%s"),
}


@functools.lru_cache(maxsize=None)
def ball_centre():
    """The point of a 0.1 grid, at least BALL_RADIUS + cutoff + MARGIN from every box face, that is farthest from every bead of
    the start."""
    s = fi.INPUTS[NAME]()["system"]
    x, _ = wrap_into_box(s)
    box = np.asarray(s["box"], dtype=np.float64)
    keep = BALL_RADIUS + WALL["cutoff"] + MARGIN
    axes = [np.arange(box[d, 0] + keep, box[d, 1] - keep, 0.1) for d in range(3)]
    assert all(len(a) for a in axes)
    best, where = -1.0, None
    for gx in axes[0]:
        g = np.stack(np.meshgrid([gx], axes[1], axes[2], indexing="ij"), axis=-1).reshape(-1, 3)
        d = np.sqrt(((g[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
        k = int(np.argmax(d))
        if d[k] > best:
            best, where = float(d[k]), g[k]
    return tuple(float(c) for c in where), best


def wall_lines():
    c, _ = ball_centre()
    return ("region hole sphere %.17g %.17g %.17g %.17g side out\n" % (c[0], c[1], c[2], BALL_RADIUS) +
            "fix w all wall/region hole lj126 %.17g %.17g %.17g\nfix_modify w energy yes virial yes\n" % (WALL["epsilon"], WALL["sigma"], WALL["cutoff"]))


def wall_script(order, steps=fc.STEPS):
    return fi.script(fi.INPUTS[NAME](), skin="0.2") + ORDERS[order][1] % wall_lines() + "thermo %d\nrun %d\n" % (THERMO, steps)


class WallSystem(fr.System):
    """force_reference.System with one wall: its force on every bead, its energy in pe / etotal, its virial in the pressure."""

    def evaluate(self, x, only=None):
        ev = super().evaluate(x, only)
        t = wr.wall_terms(x, self.wall_region, self.wall)
        assert not t["outside"].any(), "a bead inside the ball"
        self.contacts.append(int((t["ncontact"] > 0).sum()))
        self.wall_fmax.append(float(np.abs(t["f"]).max()))
        return ev._replace(f=ev.f + t["f"], terms=dict(ev.terms, wall=t))

    def thermo(self, ev, v, norm=None):
        out = super().thermo(ev, v, norm)
        t = ev.terms["wall"]
        nrm = fr.LD(self.n) if (self.norm if norm is None else norm) else fr.LD(1)
        out["pe"] = out["pe"] + t["energy"] / nrm
        out["etotal"] = out["etotal"] + t["energy"] / nrm
        vol = self.prd[0] * self.prd[1] * self.prd[2]
        out["press"] = out["press"] + (t["virial"][0] + t["virial"][1] + t["virial"][2]) / 3 / vol * fr.LD(self.units["nktv2p"])
        return out


@functools.lru_cache(maxsize=None)
def wall_reference_trajectory(fixes):
    """(system, trajectory) of the twelve steps with the wall, fixes = "nve" | "langevin" (the order of wall and thermostat is
    a matter of rounding alone: the reference adds in long double)."""
    from oracle import ranmars_stream
    s = fi.INPUTS[NAME]()["system"]
    model = fr.model_from_script(fc.run_script(NAME, fixes), s["ntypes"])
    S = WallSystem(model, s["box"], s["type"], s["mass"], s["bonds"], s.get("angles"))
    c, _ = ball_centre()
    S.wall_region, S.wall = dict(style="sphere", side="out", args=(c[0], c[1], c[2], BALL_RADIUS)), WALL
    S.contacts, S.wall_fmax = [], []
    x, img = wrap_into_box(s)
    u = ranmars_stream(fc.LANGEVIN_SEED, 3 * S.n * (fc.STEPS + 1)) if fixes == "langevin" else None
    return S, S.trajectory(x, s["v"], img, fc.STEPS, u)


def report(what, got, ref, oracle_dev, ceiling):
    err, b = fc.relerr(got, ref), fc.bound(oracle_dev, ceiling)
    print("%-34s engine %.2e  oracle (no wall) %.2e  bound %.2e" % (what, err, oracle_dev, b))
    return [] if err < b else ["%s: %.3e exceeds %.3e" % (what, err, b)]


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_twelve_steps(tmp_path, monkeypatch, shape, order):
    """Unwrapped positions, velocities and forces after the last step and the thermo rows of steps 0, 4, 8, 12 (etotal and
    press with the wall's share) against the reference; then positions and velocities after each of the steps 1 .. 11, from
    fresh runs of as many steps (as test_gpu_force.test_trajectory takes them).  Nine steps through the wall variant of the
    step kernel, the three thermo steps through the unfused kernels and k_wall.
    Measured on an MI355X, the largest over the nine cases (44 beads in contact, wall forces up to 168): after the last step x
    2.0e-15 (bound 1.0e-13), v 7.9e-13 (9.4e-12), f 2.0e-11 (1.4e-10), thermo rows 1.7e-14 (2.4e-13); after the steps 1 .. 11
    x 1.7e-15, v 8.3e-13 (bounds from 1.7e-13 after step 1, where it is 1.1e-14)."""
    set_env(monkeypatch, SHAPES[shape])
    fixes = ORDERS[order][0]
    S, ref = wall_reference_trajectory(fixes)
    dev, obuilds = fc.oracle_trajectory(NAME, fixes)
    odev = fc.oracle_states(NAME, fixes)
    # the inputs are what the test is for: the wall acts on a few dozen beads at every step with forces of the size of the
    # others', and no pair came closer to a cutoff than a hundred times what the position bound can move it
    print("beads in contact per step", S.contacts, "largest wall force component %.3g" % max(S.wall_fmax))
    assert min(S.contacts) >= 16 and max(S.wall_fmax) > 1.0
    assert float(min(ref["gaps"])) > fc.required_gap(NAME, fixes)
    system = fi.INPUTS[NAME]()["system"]
    p = run_product(wall_script(order), system, tmp_path)
    stats = {k: int(p.stat(k)) for k in STATS}
    rows = np.asarray(p.thermo_history())
    label = "%s %s" % (shape, order)
    bad = report(label + " x", S.unwrapped(p.gather("x"), p.gather("image")), ref["x"][-1], dev["x"], fc.TRAJ_CEILING["x"])
    bad += report(label + " v", p.gather("v"), ref["v"][-1], dev["v"], fc.TRAJ_CEILING["v"])
    bad += report(label + " f", p.gather("f"), ref["f"], dev["f"], fc.TRAJ_CEILING["f"])
    steps = list(range(0, fc.STEPS + 1, THERMO))
    assert [int(r[0]) for r in rows] == steps
    want = [[ref["rows"][k][key] for key in fc.ROW_KEYS] for k in steps]
    bad += report(label + " thermo rows", rows[:, 1:6], want, dev["rows"], fc.TRAJ_CEILING["rows"])
    p.close()
    assert stats["steps_fused_wall"] > 0 and stats["steps_unfused"] == len(steps) - 1
    assert stats == dict(dict.fromkeys(STATS, 0), steps_fused=9, steps_fused_wall=9, steps_unfused=3), stats
    for k in range(1, fc.STEPS):
        p = run_product(wall_script(order, steps=k), system, tmp_path)
        bad += report("%s x after step %d" % (label, k), S.unwrapped(p.gather("x"), p.gather("image")), ref["x"][k], odev[k - 1]["x"],
                      fc.TRAJ_CEILING["x"])
        bad += report("%s v after step %d" % (label, k), p.gather("v"), ref["v"][k], odev[k - 1]["v"], fc.TRAJ_CEILING["v"])
        p.close()
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# a wall on a group: the beads outside the group do not feel it
# ------------------------------------------------------------------------------------------------------------------
def two_clusters():
    """Two copies of a 216-bead lattice chain, 5.7 apart along x in a box with as much room beyond them (they fill the box in
    y and z): type 1 and type 2.  Nothing of one ever comes within a cutoff and a skin of the other."""
    a = lattice_chain(216, seed=5)
    b = lattice_chain(216, seed=6)
    L = float(a["box"][0][1])
    shift = np.array([L + 5.7, 0.0, 0.0])
    s = dict(a)
    s["x"] = np.concatenate([a["x"], b["x"] + shift])
    s["v"] = np.concatenate([a["v"], b["v"]])
    s["type"] = np.concatenate([np.ones(216, dtype=np.int32), np.full(216, 2, dtype=np.int32)])
    s["mol"] = np.concatenate([a["mol"], b["mol"] + 1])
    s["image"] = np.zeros((432, 3), dtype=np.int32)
    bb = b["bonds"].copy()
    bb[:, 1:] += 216
    s["bonds"] = np.concatenate([a["bonds"], bb])
    s["box"] = np.array([[-5.7, 2 * L + 11.4], [0.0, L], [0.0, L]])
    s["ntypes"], s["mass"] = 2, [1.0, 1.0]
    return s, L


def test_wall_on_a_group_leaves_the_others_alone(tmp_path, monkeypatch):
    """A harmonic wall whose cutoff (20) reaches every bead of both clusters from the inside of a block around them, on the
    group of the first cluster: the beads of the second keep the positions, velocities and forces of a run without the wall
    bit for bit; the first cluster's differ; every step is counted unfused.  Both runs take the unfused kernels (the run
    without a wall by LAMMPS_LE_NO_FUSE, so that the same kernels do the same arithmetic on the second cluster) and rebuild
    their lists on the same steps (neigh_modify check no)."""
    s, L = two_clusters()
    head = CHAIN_SCRIPT.replace("neigh_modify every 1 delay 1 check yes", "neigh_modify every 2 delay 0 check no")
    fixes = "fix 1 all nve\n%sfix 2 all langevin 1.0 1.0 1.0 904297\nthermo 10\nrun 40\n"
    wall = ("group first type 1\nregion room block %.17g %.17g -1.0 %.17g -1.0 %.17g side in\n" % (-5.6, 2 * L + 11.3, L + 1.0, L + 1.0) +
            "fix w first wall/region room harmonic 0.05 0.0 20.0\n")
    reg, par = wr.parse_region(wall.split("\n")[1].split()[2:]), wr.parse_wall(wall.split("\n")[2].split()[5:])
    t = wr.wall_terms(s["x"], reg, par)
    assert (t["ncontact"] >= 2).all() and not t["outside"].any()          # every bead of both clusters is within the cutoff
    assert float(np.abs(t["f"][216:]).max()) > 0.1                        # ... and the wall would push the second cluster too
    runs = {}
    for label, env, w in (("wall", {}, wall), ("none", {"LAMMPS_LE_NO_FUSE": "1"}, "")):
        set_env(monkeypatch, env)
        p = run_product(head + fixes % w, s, tmp_path)
        runs[label] = dict(x=p.gather("x"), v=p.gather("v"), f=p.gather("f"), image=p.gather("image"),
                           stats={k: int(p.stat(k)) for k in STATS}, builds=int(p.stat("neigh_builds")))
        p.close()
    a, b = runs["wall"], runs["none"]
    assert a["stats"] == dict(dict.fromkeys(STATS, 0), steps_unfused=40), a["stats"]
    assert b["stats"] == dict(dict.fromkeys(STATS, 0), steps_unfused=40), b["stats"]
    assert a["builds"] == b["builds"] >= 19, (a["builds"], b["builds"])
    for q in ("x", "v", "f", "image"):
        assert np.array_equal(a[q][216:], b[q][216:]), "%s of the beads outside the group differs" % q
    # the wall did act on its group: every member's velocity has moved
    assert (np.abs(a["v"][:216] - b["v"][:216]).max(axis=1) > 1e-6).all()
    # and no bead of one cluster came near the other
    gap = a["x"][216:, 0].min() - a["x"][:216, 0].max()
    assert gap > 4.0, gap


# ------------------------------------------------------------------------------------------------------------------
# decomposed: the LE cycle inside the WCA sphere on 2 and 3 z slabs against one rank
# ------------------------------------------------------------------------------------------------------------------
DD_STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall", "neigh_builds",
            "fene_warnings", "comm_nranks", "nlocal")          # (dd_wall_worker.STATS)


def dd_script():
    fx = wl.fixture("langevin_then_wall")
    lines = fx.scn["script"].split("\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run ") or ln.startswith("run_style"))
    lines.insert(k, "thermo_style custom " + " ".join(("step",) + rr.THERMO))
    return "\n".join(lines), fx.system()


_one = {}


def one_rank(tmp_path):
    if not _one:
        script, system = dd_script()
        p = run_product(script, system, tmp_path)
        _one.update(x=p.gather("x"), v=p.gather("v"), image=p.gather("image"), type=p.gather("type"), num_bond=p.gather("num_bond"),
                    bond_type=p.gather("bond_type"), bond_atom=p.gather("bond_atom"), rows=np.asarray(p.thermo_history(), dtype=np.float64),
                    pe=np.array([p.get_thermo("pe")]),
                    wall=np.array([p.extract_fix("w", 0, 0)] + [p.extract_fix("w", 0, 1, k) for k in range(3)]),
                    stats=np.array([p.stat(k) for k in DD_STATS], dtype=np.float64))
        for fid in ("loop", "loading", "unloading"):
            _one["f_" + fid] = np.array([p.extract_fix(fid, 0, 1, 0), p.extract_fix(fid, 0, 1, 1)])
        p.close()
    return _one


def run_wall_ranks(world, system, script, tmp_path):
    session = uuid.uuid4().hex[:12]
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out.npz"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dd_wall_worker.py"), str(r), str(world), session, sysfile,
                               scriptfile, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return np.load(out)


@pytest.mark.parametrize("world", [2, 3])
def test_walls_across_slabs(tmp_path, monkeypatch, world):
    """The recorded scenario langevin_then_wall (1000 beads, 48 steps, the three LE fixes, wall energy and virial in the thermo
    rows) on 2 and 3 slabs, one process per rank, against the same script on one rank: bond tables, types, image flags, the LE
    fixes' counters, list builds, FENE warnings and the steps' paths identical; x to 1e-9, v to 1e-8, every thermo column, pe
    and f_w, f_w[1..3] (relative to max(1, |value|)) to 1e-9 - what test_gpu_dd.py asks of slabs against the oracle.
    Measured on an MI355X (2 / 3 slabs): x 3.6e-15 / 5.3e-15, v 9.8e-14 / 1.7e-13, thermo rows 3.6e-15 / 7.1e-15, the wall's
    sums 2.4e-12 / 2.7e-12 absolute (their order of summation follows the ranks)."""
    set_env(monkeypatch, {})
    script, system = dd_script()
    one = one_rank(tmp_path)
    r = run_wall_ranks(world, system, script, tmp_path)
    st, st1 = dict(zip(DD_STATS, r["stats"])), dict(zip(DD_STATS, one["stats"]))
    assert st["comm_nranks"] == world and 0 < st["nlocal"] < len(system["x"])
    for k in DD_STATS[:7]:
        assert st[k] == st1[k], (k, st[k], st1[k])
    assert st["steps_fused_wall"] == 43 and st["steps_unfused"] == 5
    for q in ("num_bond", "bond_type", "bond_atom", "type", "image", "f_loop", "f_loading", "f_unloading"):
        assert np.array_equal(r[q], one[q]), q
    assert (r["bond_type"] == 2).sum() >= 3
    print("%d slabs: x %.2e v %.2e rows %.2e wall %.2e" % (world, np.abs(r["x"] - one["x"]).max(), np.abs(r["v"] - one["v"]).max(),
                                                          np.abs(r["rows"] - one["rows"]).max(), np.abs(r["wall"] - one["wall"]).max()))
    assert np.abs(r["x"] - one["x"]).max() < 1e-9
    assert np.abs(r["v"] - one["v"]).max() < 1e-8
    assert r["rows"].shape == one["rows"].shape and np.abs(r["rows"] - one["rows"]).max() < 1e-9
    assert abs(r["pe"][0] - one["pe"][0]) < 1e-9
    assert (np.abs(r["wall"] - one["wall"]) / np.maximum(1.0, np.abs(one["wall"]))).max() < 1e-9 and np.abs(one["wall"]).max() > 0
