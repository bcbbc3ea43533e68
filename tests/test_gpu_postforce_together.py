"""The post-force fixes of all three families in one run, through every caller of the engine's post-force sequence.

census_runs.together_script: the 2145 beads of the input `census` with a wall, a tether on a group and a pull with `every 3`
ahead of fix langevin, an indenter and a pinned group (fix setforce) behind it, `fix_modify energy yes` on the wall, the
indenter and the pull, `thermo 4` - twelve steps under run_style verlet (every plain step takes the unfused kernels: the step
kernel has no variant with a wall and the force fixes at once), under run_style respa 2 2 (without the pinned group: the engine
refuses fix setforce there) and twelve iterations of `minimize` (which ignores the thermostat; the two places stay).

Each run is held two ways:
  against the long-double restatement (force_reference.py with the fixes' terms of wall_reference, extforce_reference and
  indent_reference through its `extra` and `after` hooks; census_runs.respa_trajectory for r-RESPA) under the bounds of
  test_gpu_step_census.compare_new: 16 x the deviation of the float64 run of the same restatement, at least 1e-13, under the
  ceilings.  The minimisation, whose path no restatement of twelve steps follows, is held as test_gpu_minimize.py holds its end
  states: forces and pe at the gathered end positions against the brute force, within force_compare.RUN0_CEILING;
  bit for bit against tests/golden/postforce_together_<mode>.json, what the build of the commit before the post-force fixes got
  one owner left on an MI355X (that build reproduced itself in all three runs): every thermo row, every f_ID and f_ID[k] of the
  five fixes at every thermo step and the step counters as recorded; final positions, velocities and image flags of every bead
  through their SHA-256 (equal exactly when every element is: the doubles of three runs written out are a megabyte of text),
  and of every sixteenth bead and the pinned group value by value, as hex floats."""
import numpy as np
import pytest

import census_runs as cr
import force_compare as fc
import force_reference as fr
from test_gpu_step_census import compare_new

pytestmark = pytest.mark.gpu

_runs = {}


def run(mode, tmp_path_factory):
    if mode not in _runs:
        _runs[mode] = cr.run_together(mode, tmp_path_factory.mktemp("together_" + mode))
    return _runs[mode]


@pytest.mark.parametrize("mode", cr.MODES)
def test_against_the_record_of_the_parent(mode, tmp_path_factory):
    got, rec = run(mode, tmp_path_factory), cr.together_record(mode)
    steps = list(range(0, fc.STEPS + 1, cr.THERMO))
    assert [int(r[0]) for r in got["log"]] == steps and len(rec["columns"]) == got["log"].shape[1]
    assert got["stats"] == rec["stats"], (got["stats"], rec["stats"])
    for k, col in enumerate(rec["columns"]):
        assert np.array_equal(got["log"][:, k], rec["log"][:, k]), "%s: %r against %r recorded" % (col, list(got["log"][:, k]), list(rec["log"][:, k]))
    assert np.array_equal(got["rows"], rec["rows"])
    # the end state: the sampled beads value by value (which say where a difference lies), then every bead through the digests
    k = rec["sample"]["beads"]
    assert np.array_equal(k, cr.sample_beads(len(got["x"])))
    for q in ("x", "v", "image"):
        assert np.array_equal(got[q][k], rec["sample"][q]), "%s differs on %d of the %d sampled beads" % (q, (got[q][k] != rec["sample"][q]).any(axis=1).sum(), len(k))
    for q, dtype in (("x", np.float64), ("v", np.float64), ("image", np.int64)):
        assert cr.digest(got[q], dtype) == rec["sha256"][q], "%s differs from the record on a bead outside the sample" % q


@pytest.mark.parametrize("mode", ("verlet", "respa"))
def test_against_the_long_double_restatement(mode, tmp_path_factory):
    got = run(mode, tmp_path_factory)
    act = cr.reference("together", mode)[1]["acting"]
    assert act["w"] > 0 and act["c"] > 0 and (act["z"] > 0 or mode == "respa"), act
    assert got["stats"]["steps_unfused"] == fc.STEPS and got["stats"]["steps_fused"] == 0, got["stats"]
    compare_new("together-" + mode, "together", mode, got)


def end_state(got, step):
    """Forces with the five fixes' terms in fix order, and pe, at the gathered end state `got`, in the precision in force."""
    s = cr.system()
    x0, img0 = cr.wrap_into_box(s)
    S = cr.PrunedSystem(fr.model_from_script(cr.script("wall", False), s["ntypes"]), s["box"], s["type"], s["mass"], s["bonds"])
    x, img = got["x"], got["image"]
    moved = float(np.sqrt(((S.unwrapped(x, img) - S.unwrapped(x0, img0)) ** 2).sum(axis=1).max()))
    assert moved < cr.REACH / 2, moved          # (no pair outside census_runs.candidates() came within the cutoff)
    ev = S.evaluate(np.asarray(S.lo + np.mod(fr.ld(x) - S.lo, S.prd)))          # (between two list builds a bead may sit just outside the box)
    T = cr.Together(s, x0, img0)
    f = T.behind(step, x, img, T.ahead(step, x, img, ev.f))
    assert T.acting["w"] > 0 and T.acting["c"] > 0 and T.acting["z"] > 0, T.acting
    return f, (ev.evdwl + ev.ebond + T.efix()) / fr.LD(S.n)


def test_minimize_end_state_against_brute_force(tmp_path_factory):
    """test_gpu_minimize.test_end_state_against_brute_force for this run, with the bound of the census rows: 16 x what the float64
    run of the same restatement is off by at this state, at least 1e-13, under the ceilings of short trajectories (the state is
    the end of one).  force_compare.RUN0_CEILING, which that test holds its own inputs to, is out of reach of float64 here: the
    restatement's own float64 forces are 2.4e-12 from its long-double ones at the recorded end state (the bonds' part: terms of
    up to 66 that cancel to forces below 1).  Measured on an MI355X: forces 3.6e-12 (bound 3.8e-11), pe 0."""
    got = run("minimize", tmp_path_factory)
    step = int(got["rows"][-1, 0])
    assert step == got["stats"]["min_iterations"] == fc.STEPS and step % cr.PULL_EVERY == 0          # (the pull acts on the last evaluation)
    f, pe = end_state(got, step)
    with fr.precision(np.float64):
        f_low, pe_low = end_state(got, step)
    bf, be = fc.bound(fc.relerr(f_low, f), fc.TRAJ_CEILING["f"]), fc.bound(fc.relerr(pe_low, pe), fc.TRAJ_CEILING["rows"])
    ef, ee = fc.relerr(got["f"], f), fc.relerr(got["pe"], pe)
    print("minimize end state: forces %.2e (bound %.2e), pe %.2e (bound %.2e) off the brute force" % (ef, bf, ee, be))
    assert ef <= bf and ee <= be
