"""The CPU oracle against recorded runs of the reference program that END IN AN ERROR because one per-atom row is one slot
short (tests/golden/ref_limit_*.npz; table: reference_runs.LIMITS; recorder: tests/golden/make_reference_runs.py).

Every limit scenario is a script the reference aborts: a bond row, a special row or an angle row is exactly full and a fix wants
one entry more.  The fixture holds the error text (without the `ERROR on proc N:` prefix and the `(file:line)` suffix), the step
of the error, and the state after the last complete step.  The oracle runs to that step - integer rows exactly, x and v under
16 x the spread of the reference's own three perturbed reruns, the rule of reference_runs - and must then raise exactly the
recorded text in the next step.  The twin of a limit scenario, the same script with one slot more, is an ordinary scenario of
reference_runs.SCENARIOS and goes through test_reference_runs_cpu.py; here it is only asked to exist and to end full.

What the recordings showed (reference's text -> what the oracle and the engine said before):
  limit_load_rebuild_special  `Special list size exceeded in fix ex_load` (its own rebuild_special_one)   -> `... in fix bond/create`
  limit_ext_rebuild_special   `Special list size exceeded in fix bond/create` (fix extrusion's copy says so) -> the same
  limit_load_bpa / _special   `New bond exceeded ... in fix ex_load`                                       -> the same
  limit_create_bpa / _special `New bond exceeded ... in fix bond/create`                                   -> the same
  limit_load_angles, limit_ext_multi, limit_ext_bpa_low                                                    -> the same
  limit_ext_bpa_high          no error: the reference runs on with bond 250-252 stored by bead 250 alone   -> the oracle follows

Rows of the issue's table that are not here, and why:
  - limit_load_special has no twin: with `special_bonds fene` an untouched bead lists its 1-2 partners only, so the insert
    overflows only when the row holds exactly those two; one slot more lets the insert pass and the rebuild that follows (7
    entries) overflows instead - which is limit_load_rebuild_special.  After a rebuild the partner of a new (i, i+2) bond is
    always in the 1-3 block already, so the insert cannot overflow a longer row.  The same holds for limit_create_special.
  - limit_ext_multi has no capacity to enlarge.
  - limit_create_special is the insert (`extra special per atom` 0); the rebuild overflow of bond/create goes through the same
    code as ex_load's, which limit_load_rebuild_special and its twin hold."""
import json
import os

import numpy as np
import pytest

import reference_runs as rr
from systems import OracleScript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")


def oracle_to_the_last_complete_step(name):
    """(the OracleScript after `run S`, the dict check_discrete takes)"""
    fx = rr.fixture(name)
    s = fx.system()
    run = OracleScript(s)
    o = run.run(rr.script_for_steps(fx.scn, fx.last))
    if fx.last == 0:
        o.run(0)          # (setup: the forces and the thermo row of step 0)
    nb, bt, ba = o.bond_table()
    got = dict(bond=rr.bond_rows(nb, bt, ba), angle=None, type=o.types().copy(), image=o.image().copy(), x=o.x(), v=o.v(),
               bonds=float(o.nbonds()), fixvec={fid: tuple(float(q) for q in o.fix_vector(fid)) for fid in fx.scn["fixes"]}, num_bond=nb)
    if rr.has_angles(fx.scn):
        got["angle"], got["angles"] = rr.angle_rows(*o.angle_table()), float(o.nangles())
    r = o.thermo_history()[-1]
    got["row"] = dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5])
    return run, got


def compare_last_complete_step(fx, got, label, oracle=None):
    """oracle: the oracle's own dict for the same step (the GPU tests pass it: their second bound, as in test_gpu_reference_runs.py)."""
    bad = rr.check_discrete(fx, fx.last, got)
    if not np.array_equal(got["num_bond"], fx.z["num_bond"]):
        bad.append("per-atom bond counts differ from the recorded ones")
    odev = rr.deviation(fx, fx.last, oracle["x"], oracle["image"], oracle["v"]) if oracle else None
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"]), label, odev)
    assert got["row"]["step"] == fx.last == int(fx.thermo()[0, 0])
    for nm in ("temp", "epair", "emol", "etotal", "press"):
        want = fx.thermo()[0, fx.col(nm)]
        err = abs(got["row"][nm] - want)
        b = rr.thermo_bound(fx, 0, nm, abs(oracle["row"][nm] - want) if oracle else 0.0)
        if not err <= b:
            bad.append("%s thermo %s after step %d: %.3e exceeds %.3e" % (label, nm, fx.last, err, b))
    return bad


@pytest.mark.parametrize("name", rr.ERROR_LIMITS)
def test_oracle_stops_where_the_reference_stops(name):
    """run S: the state of the last complete step.  run 1: the recorded text, raised in step S + 1."""
    fx = rr.fixture(name)
    run, got = oracle_to_the_last_complete_step(name)
    bad = compare_last_complete_step(fx, got, name)
    assert not bad, "\n".join(bad)
    with pytest.raises(RuntimeError) as e:
        run.o.run(1)
    assert str(e.value) == fx.error
    assert run.o.ntimestep() == fx.error_step


@pytest.mark.parametrize("name", rr.ERROR_LIMITS)
def test_oracle_rows_before_the_error(name):
    """Fresh oracle runs up to every earlier step at which the reference's rows changed."""
    fx = rr.fixture(name)
    steps = set(fx.change_steps()) | (set(fx.change_steps("angle")) if rr.has_angles(fx.scn) else set())
    bad = []
    for step in sorted(steps - {0, fx.last}):
        bad += rr.check_discrete(fx, step, rr.oracle_run(name, step))
    assert not bad, "\n".join(bad)


def test_oracle_follows_the_one_sided_bond():
    """limit_ext_bpa_high: bead 252 is full, bead 250 is not; the reference stores the new bond 250-252 at bead 250 alone, counts
    one created and one broken bond, and runs on.  The oracle ends where that run ends, one-sided bond included (the rows list a
    bond from the end that stores it; the per-atom counts show that 252 does not)."""
    name = "limit_ext_bpa_high"
    fx = rr.fixture(name)
    got = rr.oracle_run(name)
    bad = rr.check_discrete(fx, fx.last, got)
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), name)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], ("temp", "epair", "emol", "etotal", "press")), name)
    assert not bad, "\n".join(bad)
    from systems import run_oracle
    nb = run_oracle(fx.scn["script"], fx.system()).bond_table()[0]
    assert np.array_equal(nb, fx.z["num_bond"])
    assert [2, 250, 252] in fx.rows_at(fx.last).tolist() and nb[249] == 2 and nb[251] == 2 and rr.capacities(fx.system())["bond"] == 2
    for step in fx.change_steps():
        if 0 < step < fx.last:
            assert rr.check_discrete(fx, step, rr.oracle_run(name, step)) == []


# ------------------------------------------------------------------------------------------------------------------
# the fixtures themselves
# ------------------------------------------------------------------------------------------------------------------
def test_limit_fixture_conditions():
    """What the generator refuses to write, asked of the committed files: one kind of ERROR, the same text at the same step in
    the three perturbed reruns with the same rows before it, the bead at its limit after the last complete step, and the twin
    - the same script, one slot more - recorded to its end with a full row.  At most 2048 beads and 48 steps (60 where the
    twin is an older scenario of 60)."""
    meta = json.load(open(os.path.join(rr.GOLDEN, "ref_runs.json")))
    assert sorted(meta["limits"]) == sorted(rr.LIMIT_NAMES)
    texts = set()
    for name in rr.LIMIT_NAMES:
        fx = rr.fixture(name)
        assert rr.limit_conditions(fx) == "", (name, rr.limit_conditions(fx))
        assert fx.scn["system"]["n"] <= 2048 and fx.scn["checkpoints"][-1] <= 60
        if fx.scn["runs_on"]:
            assert fx.error is None
            continue
        assert fx.error and "ERROR" not in fx.error and "(" not in fx.error and ".cpp" not in fx.error, fx.error
        assert fx.error_step == fx.last + 1 <= 48
        texts.add(fx.error)
        if fx.scn["twin"]:
            tw = rr.fixture(fx.scn["twin"])
            assert rr.fixture_conditions(tw) == "" and tw.last >= fx.error_step
    assert len(texts) == 9          # every error scenario ends in another text


def test_limit_data_files_are_the_recorded_ones(tmp_path):
    import hashlib
    from systems import write_data
    for name in rr.LIMIT_NAMES:
        fx = rr.fixture(name)
        path = os.path.join(str(tmp_path), "data.chain")
        write_data(path, fx.system())
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == fx.meta["data_sha256"], name


def test_twins_end_full_in_the_oracle():
    """The twins' point from the other side: at the end of the oracle's run the largest row is exactly as long as the table
    (bond_per_atom, maxspecial, angle_per_atom as the oracle holds them), which is what reached() derived from the recorded
    rows and the data file."""
    from systems import run_oracle
    seen = set()
    for name in rr.ERROR_LIMITS:
        tw = rr.LIMIT_BY_NAME[name]["twin"]
        if not tw or tw in seen:
            continue
        seen.add(tw)
        fx = rr.fixture(tw)
        o = run_oracle(fx.scn["script"], fx.system())
        cap = rr.capacities(fx.system())
        assert (o.L.leo_bond_per_atom(o.h), o.L.leo_maxspecial(o.h)) == (cap["bond"], cap["special"]), tw
        for point in fx.scn["point"].split("+"):
            if point == "full_bond":
                assert o.bond_table()[0].max() == cap["bond"], tw
            if point == "full_special":
                assert o.special_table()[0][:, 2].max() == cap["special"], tw
            if point == "full_angle":
                assert o.L.leo_angle_per_atom(o.h) == cap["angle"] and o.angle_table()[0].max() == cap["angle"], tw
    assert len(seen) == 6
