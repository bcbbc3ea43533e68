"""Every instantiation of the step kernel the engine can launch, launched next to a reference, and counted.

k_step exists in 177 instantiations (csrc/step_plan.h step_variant_exists); Engine::iterate can launch 93 of them (LIVE,
test_step_census_cpu.py).  The other modules know the instantiation a run took by family alone (lammps_le_stat steps_fused*).
Here every row of CASES names the exact set of k_step and k_force instantiations its run must launch - by the key of the
engine's launch census (step_census.py) - runs through the C-ABI on a fresh handle, compares the end state with a reference and
then holds the handle's census against the row: no key missing, none besides, none outside LIVE.  The union of the rows' keys
is LIVE and the k_force instantiations the engine can launch; test_step_census_cpu.py asserts that from the table, without a GPU.

The rows and their references:
  fc       the twelve-step inputs of force_inputs.py under force_compare's scripts, compared by test_gpu_force.compare_trajectory
           (long-double reference; bound 16 x the FP64 oracle's deviation, at least 1e-13, under the ceilings; list builds against
           the oracle's): the base family with a pair style, angles, fixes on groups, the energy variant, the variants that take
           pending velocities, the diagnostic launch
  new      census_runs.py: 2145 beads with a wall, an indenter, a tether and a pull, pair_style soft or no pair style, with and
           without fix langevin, in the three lane shapes; bound 16 x the deviation of the float64 run of the same restatement;
           list builds against the reference trajectory's own displacement rule
  recorded the r-RESPA runs of extforce_runs.py and soft_runs.py through their own modules' runners and comparisons (k_force
           with the pair part alone)
`relabel`: the same beads under shuffled IDs (census_runs.relabelled) - the rank-table order (I = 0) of an input whose file is
in ID order (I = 1); what the engine hands out by ID is put back into the reference's order before it is compared."""
import numpy as np
import pytest

import census_runs as cr
import force_compare as fc
import force_inputs as fi
import step_census as sc
from step_census import force_key, key
from systems import run_product

pytestmark = pytest.mark.gpu

PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD}
SHAPE_FLAGS = {"four": dict(LPB=4, AHEAD=1), "plain": dict(LPB=1, AHEAD=0), "ahead": dict(LPB=1, AHEAD=1)}
UNFUSED = {"LAMMPS_LE_NO_FUSE": "1"}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
THERMO = 4
PLAIN_STEPS, THERMO_STEPS = 9, 3          # twelve steps with `thermo 4`: thermo steps 4, 8, 12
ANY = None                                # a count the row does not determine (at least one launch)


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
CASES = {}


def row(cid, **kw):
    assert cid not in CASES
    kw.setdefault("sums", [])
    CASES[cid] = kw


def twelve(step_key, pair=1, soft=0, fused_thermo=None):
    """The census of twelve steps with `thermo 4` whose plain steps take `step_key`: nine launches of it; the thermo steps
    take the energy variant `fused_thermo` or k_force<E> - which the setup of every run launches once as well."""
    step = {step_key: PLAIN_STEPS}
    if fused_thermo is not None:
        step[fused_thermo] = THERMO_STEPS
    return step, {force_key(E=1, P=pair, SOFT=soft): 1 + (0 if fused_thermo is not None else THERMO_STEPS)}


# base family with a pair style: `offset` (630 beads) under force_compare's scripts.  The one-lane shape without look-ahead is
# the one with an energy variant (thermo steps) and the one that takes the velocities a rebuild left pending (the step behind
# a rebuild that falls on a plain step): its nine plain launches are shared between the two keys
for L, fixes in ((0, "nve"), (1, "langevin")):
    for I in (1, 0):
        for shape in SHAPES:
            k = key(L=L, N=1, I=I, P=1, **SHAPE_FLAGS[shape])
            if shape == "plain":
                lazy = key(L=L, N=1, I=I, P=1, LAZYV=1)
                step, force = twelve(k, fused_thermo=key(L=L, I=I, P=1, EF=1))
                step[k] = ANY
                step[lazy] = ANY
                sums = [((k, lazy), PLAIN_STEPS)]
            else:
                (step, force), sums = twelve(k), []
            row("base-%s-%s-%s" % (fixes, "ident" if I else "ranks", shape), kind="fc", input="offset", fixes=fixes, relabel=not I,
                env=SHAPES[shape], step=step, force=force, sums=sums)

# angles inside the step: `angles-harmonic`, with and without look-ahead (four lanes per bead have no angle variant: the
# planner answers a request for them with the look-ahead shape)
for L, fixes in ((0, "nve"), (1, "langevin")):
    for I in (1, 0):
        for shape in ("plain", "ahead"):
            step, force = twelve(key(L=L, N=1, I=I, P=1, ANG=1, AHEAD=SHAPE_FLAGS[shape]["AHEAD"]))
            row("angles-%s-%s-%s" % (fixes, "ident" if I else "ranks", shape), kind="fc", input="angles-harmonic", fixes=fixes,
                relabel=not I, env=SHAPES[shape], step=step, force=force)

# fix nve on a group (every seventh bead pinned; on the angle input the group holds every bead - the group variant all the
# same): one lane, no look-ahead, the rank table whatever the order
for L, fixes in ((0, "group"), (1, "group-langevin")):
    for ANG, name in ((0, "offset-pinned"), (1, "angles-harmonic")):
        step, force = twelve(key(L=L, N=1, P=1, GRP=1, ANG=ANG))
        row("group-%s-%s" % (fixes, "angles" if ANG else "bonds"), kind="fc", input=name, fixes=fixes, relabel=False, env=PLAIN,
            step=step, force=force)

# the diagnostic launch: LAMMPS_LE_DIAG_STEP with one bit set puts <L, N, I, P, 1, DIAG> in front of every plain launch.  The
# end state is bit for bit that of base-langevin-ident-plain; the census is that run's plus the DIAG key - but for the
# pending velocities, which a launch behind a diagnostic launch does not take (step_plan.h takes_pending_v): all nine plain
# launches are the plain key's
step, force = twelve(key(L=1, N=1, I=1, P=1), fused_thermo=key(L=1, I=1, P=1, EF=1))
step[key(L=1, N=1, I=1, P=1, DIAG=1)] = PLAIN_STEPS
row("diag", kind="fc", input="offset", fixes="langevin", relabel=False, env=dict(PLAIN, LAMMPS_LE_DIAG_STEP="2"), step=step, force=force,
    twin="base-langevin-ident-plain")

# the families of census_runs.py, 2145 beads: no pair style (base family, P = 0), wall, soft, tether and pull, indenter
FAMILY_FLAGS = {"nopair": dict(P=0), "wall": dict(P=1, WALL=1), "soft": dict(P=1, SOFT=1), "ext": dict(P=1, EXT=1),
                "indent": dict(P=1, WALL=1, INDENT=1)}
for family in cr.FAMILIES:
    for L in (0, 1):
        for I in (1, 0):
            for shape in SHAPES:
                fl = FAMILY_FLAGS[family]
                step, force = twelve(key(L=L, N=1, I=I, **fl, **SHAPE_FLAGS[shape]), pair=fl["P"], soft=fl.get("SOFT", 0))
                row("%s-%s-%s-%s" % (family, "langevin" if L else "nve", "ident" if I else "ranks", shape), kind="new", family=family,
                    langevin=L, relabel=not I, env=SHAPES[shape], step=step, force=force)

# k_force without the step kernel: every step of a run under LAMMPS_LE_NO_FUSE takes k_force<E = 0>, thermo steps and setup <E = 1>
row("unfused-lj", kind="fc", input="offset", fixes="nve", relabel=False, env=UNFUSED, step={},
    force={force_key(P=1): PLAIN_STEPS, force_key(E=1, P=1): 1 + THERMO_STEPS})
row("unfused-soft", kind="new", family="soft", langevin=0, relabel=False, env=UNFUSED, step={},
    force={force_key(P=1, SOFT=1): PLAIN_STEPS, force_key(E=1, P=1, SOFT=1): 1 + THERMO_STEPS})
row("unfused-nopair", kind="new", family="nopair", langevin=0, relabel=False, env=UNFUSED, step={},
    force={force_key(): PLAIN_STEPS, force_key(E=1): 1 + THERMO_STEPS})
# ... and the pair part alone: r-RESPA with the pair style on the outer level (the bonds' level takes <P = 0>; setup and thermo
# steps take their energies from a whole evaluation, <E P>), recorded runs
row("respa-lj", kind="recorded", module="extforce", name="respa2", env={}, step={},
    force={force_key(P=1, NOBOND=1): ANY, force_key(): ANY, force_key(E=1, P=1): ANY})
row("respa-soft", kind="recorded", module="soft", name="respa", env=PLAIN, step={},
    force={force_key(P=1, NOBOND=1, SOFT=1): ANY, force_key(): ANY, force_key(E=1, P=1, SOFT=1): ANY})


def table_keys(kernel):
    """The union of the rows' keys - over the table, not over what ran."""
    return set().union(*[set(c["force" if kernel == sc.FORCE else "step"]) for c in CASES.values()])


# ------------------------------------------------------------------------------------------------------------------
# the runs
# ------------------------------------------------------------------------------------------------------------------
def state_of(p, perm=None):
    """What a run leaves, by ID - in the reference's order where the IDs were shuffled."""
    got = dict(x=p.gather("x"), v=p.gather("v"), image=p.gather("image"), f=p.gather("f"))
    if perm is not None:
        got = {q: a[perm] for q, a in got.items()}
    got.update(rows=np.asarray(p.thermo_history()), builds=int(p.stat("neigh_builds")), step=sc.census(p, sc.STEP), force=sc.census(p, sc.FORCE))
    return got


def run_fc(c, tmp_path):
    system = fi.INPUTS[c["input"]]()["system"]
    perm = None
    if c["relabel"]:
        system, perm = cr.relabelled(system)
    p = run_product(fc.run_script(c["input"], c["fixes"], THERMO), system, tmp_path)
    try:
        return state_of(p, perm)
    finally:
        p.close()


def run_new(c, tmp_path):
    system, perm = cr.system(), None
    if c["relabel"]:
        system, perm = cr.relabelled(system)
    p = run_product(cr.script(c["family"], c["langevin"]), system, tmp_path)
    try:
        return state_of(p, perm)
    finally:
        p.close()


def compare_new(label, family, langevin, got):
    """test_gpu_force.compare_trajectory for a run of census_runs.py: the float64 restatement in the oracle's place."""
    from test_gpu_force import report
    S, ref, dev, builds = cr.reference(family, langevin)
    if family != "nopair":
        assert float(min(ref["gaps"])) > cr.required_gap(S, dev)
    bad = report(label + " x", S.unwrapped(got["x"], got["image"]), ref["x"][-1], dev["x"], fc.TRAJ_CEILING["x"])
    bad += report(label + " v", got["v"], ref["v"][-1], dev["v"], fc.TRAJ_CEILING["v"])
    bad += report(label + " f", got["f"], ref["f"], dev["f"], fc.TRAJ_CEILING["f"])
    steps = list(range(0, fc.STEPS + 1, THERMO))
    assert [int(r[0]) for r in got["rows"]] == steps, got["rows"][:, 0]
    want = [[ref["rows"][k][q] for q in fc.ROW_KEYS] for k in steps]
    bad += report(label + " thermo rows", got["rows"][:, 1:6], want, dev["rows"], fc.TRAJ_CEILING["rows"])
    assert not bad, "\n".join(bad)
    assert len(builds) >= 3 and got["builds"] == len(builds), (got["builds"], builds)
    check_image(S, ref, builds, got)


def check_image(S, ref, builds, got):
    """Image flags exactly: those of the reference at the last list build (census_runs.image_flags)."""
    want, margin = cr.image_flags(S, ref["x"], builds)
    assert margin > 1e-9, margin          # (no coordinate at a face on that step)
    assert np.array_equal(got["image"], want), "image flags differ on %d beads" % (got["image"] != want).any(axis=1).sum()


def run_recorded(c, tmp_path, monkeypatch):
    """A recorded run through its module's own runner and comparison; the runners close their handle, so the census is read on
    the way into close()."""
    from lammps_le_amd import lammps
    seen = []
    close = lammps.close

    def closing(self):
        if self.lmp:
            seen.append((sc.census(self, sc.STEP), sc.census(self, sc.FORCE)))
        close(self)
    monkeypatch.setattr(lammps, "close", closing)
    if c["module"] == "extforce":
        import test_gpu_extforce as m
        got = m.engine_run(c["name"], tmp_path)
        bad = m.compare_end(c["name"], got, c["name"])
        assert not bad, "\n".join(bad)
    else:
        import test_gpu_soft as m
        m.test_steps_against_recorded_runs(tmp_path, monkeypatch, c["name"], "plain")
    assert len(seen) == 1
    return dict(step=seen[0][0], force=seen[0][1])


def check_census(cid, c, got):
    bad = []
    for kernel, what in ((sc.STEP, "step"), (sc.FORCE, "force")):
        have, want = got[what], c[what]
        print(cid, what, {sc.name(k, kernel): n for k, n in sorted(have.items())})
        if set(have) - set(want):
            bad.append("launched but not expected: " + sc.names(set(have) - set(want), kernel))
        if set(want) - set(have):
            bad.append("expected but not launched: " + sc.names(set(want) - set(have), kernel))
        for k, n in want.items():
            if n is not ANY and k in have and have[k] != n:
                bad.append("%s: %d launches, %d expected" % (sc.name(k, kernel), have[k], n))
    for keys, n in c["sums"]:
        if sum(got["step"].get(k, 0) for k in keys) != n:
            bad.append("%s: %d launches together expected" % (sc.names(keys), n))
    outside = set(got["step"]) - sc.live_keys()
    if outside:
        bad.append("launched, but not in LIVE (the model of test_step_census_cpu.py is wrong): " + sc.names(outside))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cid", list(CASES))
def test_census(tmp_path, monkeypatch, cid):
    """Run, compare, check the census (see the module's text).
    Measured on an MI355X, the largest over the rows (engine / what stands in the oracle's place / smallest bound): the fc rows x
    3.6e-15 / 3.6e-15 / 1.0e-13, v 8.6e-13 / 8.6e-13 / 9.4e-12, f 2.2e-11 / 2.2e-11 / 1.4e-10, thermo rows 3.1e-14 / 5.6e-14 /
    1.7e-13; the rows of census_runs.py (the float64 restatement in the oracle's place) x 1.5e-15 / 1.5e-15 / 1.0e-13, v 9.5e-13 /
    9.5e-13 / 8.1e-12, f 3.7e-11 / 3.7e-11 / 1.7e-10, thermo rows 4.1e-14 / 4.3e-14 / 1.0e-13; no quantity of any row above 0.07
    of its bound.  The r-RESPA rows: their own modules' figures.  Every census equal to its row; no instantiation got its first
    compared launch here with anything wrong in it.  90 rows in 11 s."""
    c = CASES[cid]
    set_env(monkeypatch, c["env"])
    if c["kind"] == "fc":
        from test_gpu_force import compare_trajectory
        got = run_fc(c, tmp_path)
        compare_trajectory(cid, c["input"], c["fixes"], THERMO, got["x"], got["v"], got["image"], got["f"], got["rows"], got["builds"])
        ref = fc.reference_trajectory(c["input"], c["fixes"])
        builds, margin = cr.list_builds(ref["x"])
        assert margin > 1e-9 and len(builds) == got["builds"], (builds, got["builds"])
        check_image(fc.reference_system(c["input"], c["fixes"])[0], ref, builds, got)
    elif c["kind"] == "new":
        got = run_new(c, tmp_path)
        compare_new(cid, c["family"], c["langevin"], got)
    else:
        got = run_recorded(c, tmp_path, monkeypatch)
    if c.get("twin"):
        # the diagnostic launch changes nothing: bit for bit the run without the switch
        t = CASES[c["twin"]]
        set_env(monkeypatch, t["env"])
        twin = run_fc(t, tmp_path)
        for q in ("x", "v", "f", "image", "rows"):
            assert np.array_equal(got[q], twin[q]), "%s differs from the run without LAMMPS_LE_DIAG_STEP" % q
        assert got["builds"] == twin["builds"]
    check_census(cid, c, got)
