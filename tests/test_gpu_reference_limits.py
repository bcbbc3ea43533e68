"""The HIP path against recorded runs of the reference program that end in an error because one per-atom row is one slot short
(tests/golden/ref_limit_*.npz; table and conditions: reference_runs.LIMITS; the CPU oracle on the same fixtures:
test_reference_limits_cpu.py, whose docstring lists what the recordings showed).  Nothing here reads the reference.

Per limit scenario, in the default shape of the step kernel and with the unfused kernels: the engine runs to the last complete
step - rows, per-atom bond counts, types, image flags, counts and fix vectors exactly, x, v and the thermo row under 16 x
max(recorded spread, oracle deviation), the bounds of test_gpu_reference_runs.py -, the next step raises LammpsError with
exactly the recorded text, the step counter stands at the recorded step, and close() leaves no device block, stream or event.
These runs end in a Python exception that the host raises from a flag word, like the `Bad FENE bond` tests: every kernel they
reach checks the row's length before it stores (kernels_le.hip k_exload_create, dev_special_insert12, dev_rebuild_special_one,
dev_create_angles, k_ext_create).

limit_ext_bpa_high is the one run the engine does not follow: the reference skips the full higher end of a new extruder bond
without a word, its counts agree, and it runs on with the bond stored by the lower end alone (recorded to the end, the oracle
follows it).  The engine evaluates a bond on each end from that end's own table, so it stops at that firing with an error of
its own (ERR_ONE_SIDED) instead of running on with other forces: asserted here at the recorded firing step.

Measured on an MI355X (the last complete step; engine / oracle / recorded spread / bound): the largest are those of
limit_ext_rebuild_special after step 44, x 5.3e-15 / 5.3e-15 / 1.4e-14 / 2.3e-13 and v 2.2e-13 / 1.2e-13 / 2.8e-13 / 4.4e-12; the
scenarios that stop in step 1 compare the start itself (0).  Every text and step equal to the recorded ones in both shapes; the
22 tests of this file take 6 s.  A scratch build with three in-bounds mutations (another fix's name in the angle text, the bond
row's guard in k_exload_create firing one slot early, k_ext_create counting a new bond at its higher end) fails 15 of them and
every twin of test_gpu_reference_runs.py."""
import ctypes
import gc
import threading
import uuid

import numpy as np
import pytest

import reference_runs as rr
from systems import OracleScript, run_product, write_data
from test_gpu_reference_runs import SHAPES, set_env
from test_reference_limits_cpu import compare_last_complete_step, oracle_to_the_last_complete_step

pytestmark = pytest.mark.gpu

ONE_SIDED = "fix extrusion: a new bond would be stored by one end only (bonds per atom)"
TRANSPORT = "communicator|no answer"          # what a rank raises when another rank of its run has stopped (test_gpu_fuzz.py)


def live():
    from lammps_le_amd import library_path
    gc.collect()
    out = (ctypes.c_longlong * 3)()
    ctypes.CDLL(library_path()).lammps_le_test_live_resources(out)
    return tuple(out)


_oracle = {}


def oracle_state(name):
    if name not in _oracle:
        _oracle[name] = oracle_to_the_last_complete_step(name)[1]
    return _oracle[name]


def engine_to_the_last_complete_step(name, tmp_path):
    """(the open handle after `run S`, the dict check_discrete takes)"""
    fx = rr.fixture(name)
    lines = rr.script_for_steps(fx.scn, fx.last).split("\n")
    if fx.last == 0:
        lines.append("run 0")
    k = next(i for i, ln in enumerate(lines) if ln.startswith("run "))
    lines.insert(k, "thermo_style custom " + " ".join(("step",) + rr.THERMO))
    p = run_product("\n".join(lines), fx.system(), tmp_path)
    nb = p.gather("num_bond")
    got = dict(bond=rr.bond_rows(nb, p.gather("bond_type"), p.gather("bond_atom")), angle=None, type=p.gather("type"),
               image=p.gather("image"), x=p.gather("x"), v=p.gather("v"), bonds=float(p.get_thermo("bonds")), num_bond=nb,
               fixvec={fid: (float(p.extract_fix(fid, 0, 1, 0)), float(p.extract_fix(fid, 0, 1, 1))) for fid in fx.scn["fixes"]})
    if rr.has_angles(fx.scn):
        got["angle"] = rr.angle_rows(p.gather("num_angle"), p.gather("angle_type"), p.gather("angle_atom1"), p.gather("angle_atom2"),
                                     p.gather("angle_atom3"))
        got["angles"] = float(p.extract_setting("nangles"))
    r = p.thermo_history()[-1]
    got["row"] = dict(step=int(r[0]), temp=r[1], epair=r[2], emol=r[3], etotal=r[4], press=r[5])
    return p, got


@pytest.mark.parametrize("shape", ["default", "unfused"])
@pytest.mark.parametrize("name", rr.ERROR_LIMITS)
def test_engine_stops_where_the_reference_stops(tmp_path, monkeypatch, name, shape):
    """run S, run 1 -> the recorded text at the recorded step; nothing is left behind."""
    from lammps_le_amd import LammpsError
    set_env(monkeypatch, SHAPES[shape])
    fx, o = rr.fixture(name), oracle_state(name)
    before = live()
    p, got = engine_to_the_last_complete_step(name, tmp_path)
    try:
        bad = compare_last_complete_step(fx, got, "%s %s" % (name, shape), o)
        assert not bad, "\n".join(bad)
        with pytest.raises(LammpsError) as e:
            p.command("run 1")
        assert str(e.value) == fx.error
        assert int(p.get_thermo("step")) == fx.error_step
        assert p.stat("device_bytes") > 0
    finally:
        p.close()
    assert live() == before


@pytest.mark.parametrize("shape", ["default", "unfused"])
def test_engine_stops_at_the_one_sided_bond(tmp_path, monkeypatch, shape):
    """limit_ext_bpa_high: the firing at which the reference stores bond 250-252 at bead 250 alone (the first step at which its
    recorded rows change) ends in the engine's own error, and the step counter stands there."""
    from lammps_le_amd import LammpsError
    set_env(monkeypatch, SHAPES[shape])
    fx = rr.fixture("limit_ext_bpa_high")
    firing = fx.change_steps()[1]
    assert [2, 250, 252] in fx.rows_at(firing).tolist() and [2, 250, 252] not in fx.rows_at(firing - 1).tolist()
    before = live()
    p = run_product(rr.script_for_steps(fx.scn, firing - 1) + "run 0\n", fx.system(), tmp_path)
    try:
        assert np.array_equal(rr.bond_rows(p.gather("num_bond"), p.gather("bond_type"), p.gather("bond_atom")), fx.rows_at(firing - 1))
        with pytest.raises(LammpsError) as e:
            p.command("run 1")
        assert str(e.value) == ONE_SIDED
        assert int(p.get_thermo("step")) == firing
    finally:
        p.close()
    assert live() == before


def test_two_ranks_raise(tmp_path, monkeypatch):
    """limit_load_bpa on two z slabs (threads of this process, in-process transport): every rank raises, at least one of them
    the recorded text and the others that or the transport's abort text, and the call returns: no rank is left waiting."""
    from lammps_le_amd import lammps
    set_env(monkeypatch, {})
    fx = rr.fixture("limit_load_bpa")
    path, session, world = str(tmp_path / "data.local"), uuid.uuid4().hex[:12], 2
    write_data(path, fx.system())
    raised, steps = [None] * world, [None] * world

    def work(rank):
        lmp = lammps(cmdargs=["-screen", "none"])
        try:
            lmp.comm_init("local", rank, world, session=session)
            for ln in fx.scn["script"].split("\n"):
                w = ln.split("#")[0].split()
                lmp.command("read_data " + path if w and w[0] == "read_data" else ln)
        except Exception as e:
            raised[rank] = str(e)
            steps[rank] = int(lmp.get_thermo("step"))
        finally:
            lmp.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(m is not None for m in raised), raised
    assert fx.error in raised, raised
    import re
    assert all(m == fx.error or re.search(TRANSPORT, m) for m in raised), raised
    assert [s for s, m in zip(steps, raised) if m == fx.error] == [fx.error_step] * raised.count(fx.error)


# ------------------------------------------------------------------------------------------------------------------
# two kinds of error in one firing
# ------------------------------------------------------------------------------------------------------------------
def test_two_errors_in_one_firing(tmp_path, monkeypatch):
    """The angle scenario with a special row two slots short AND an angle row with no free slot: the first ex_load firing
    that creates a bond overflows the rebuild of a special row and the angle rows, on different beads.  The reference's
    update_topology stops inside its loop at the first rebuild that overflows and reports the angle overflow only after the
    loop (fix_ex_load.cpp:818 before :755), so the oracle says `Special list size exceeded in fix ex_load`; on the device both
    codes are raised by different lanes of one kernel, and the rank order of kernels_le.hip (le_error_rank) keeps the rebuild's,
    whichever lane stores last: the engine can match the oracle here, and must, in both shapes."""
    from lammps_le_amd import LammpsError
    scn = dict(rr.LIMIT_BY_NAME["limit_load_angles"], system=dict(rr.LIMIT_BY_NAME["limit_load_angles"]["system"], extra_special=4, extra_angle=0))
    system = rr.build_system(scn)
    run = OracleScript(system)
    with pytest.raises(RuntimeError) as eo:
        run.run(scn["script"])
    assert str(eo.value) == "Special list size exceeded in fix ex_load"
    step = run.o.ntimestep()
    # both kinds are there: with room in the special rows the same firing ends in the angle error
    other = OracleScript(rr.build_system(dict(scn, system=dict(scn["system"], extra_special=20))))
    with pytest.raises(RuntimeError, match="Fix ex_load induced too many angles"):
        other.run(scn["script"])
    assert other.o.ntimestep() == step
    for shape in ("default", "unfused"):
        set_env(monkeypatch, SHAPES[shape])
        before = live()
        p = run_product(rr.script_for_steps(scn, 0), system, tmp_path)          # (everything in front of the run command)
        try:
            with pytest.raises(LammpsError) as e:
                p.command("run %d" % scn["checkpoints"][-1])
            assert str(e.value) == str(eo.value), shape
            assert int(p.get_thermo("step")) == step
        finally:
            p.close()
        assert live() == before
