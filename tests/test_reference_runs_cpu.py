"""The CPU oracle against recorded runs of the reference program (tests/golden/ref_*.npz, scenario table: reference_runs.py).

Every other test of fix langevin, RanMars, the USER-LE fixes and their src/MC parents, the list-build schedule and the Atom::sort
order compares the HIP path with oracle/le_oracle.c - the same reading of the reference by the same hands.  Here the other
side is the reference binary itself, run once by tests/golden/make_reference_runs.py on the very
script text and data files these tests hand to the oracle: bond and angle rows after every step that changed them, types,
image flags, local order, bond / angle counts, the fix vectors and the list-build count exactly; positions, velocities, forces
and thermo columns under 16 x the reference's own spread (three reruns from starts moved by one ulp per coordinate), which is
what the GPU suite (test_gpu_reference_runs.py) then asks of the engine through the same comparison code.

Measured (oracle deviation / recorded spread, the largest over the scenarios, after the last step): x 1.2e-14 / 5.0e-14, v 3.0e-13
/ 5.2e-13, f 2.4e-11 / 4.0e-11; per scenario the oracle sits at 0.2 - 1.1 x the spread."""
import ctypes
import json
import os

import numpy as np
import pytest

import reference_runs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")
CONTINUOUS = ("temp", "epair", "emol", "etotal", "press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")


@pytest.mark.parametrize("name", rr.NAMES)
def test_oracle_ends_where_the_reference_ends(name):
    """The whole run: discrete state exactly, continuous state under 16 x the recorded spread."""
    fx = rr.fixture(name)
    got = rr.oracle_run(name)
    bad = rr.check_discrete(fx, fx.last, got)
    if got["builds"] != fx.z["builds"][-1]:
        bad.append("list builds of the last run: %d against %d recorded" % (got["builds"], fx.z["builds"][-1]))
    if not np.array_equal(got["local_order"], fx.z["local_order"]):
        bad.append("local order differs from the recorded one")
    bad += rr.check_continuous(fx, fx.last, rr.deviation(fx, fx.last, got["x"], got["image"], got["v"], got["f"]), name)
    bad += rr.check_thermo(fx, rr.thermo_deviation(fx, got["rows"], CONTINUOUS), name)
    th = fx.thermo()
    assert [r["bonds"] for r in got["rows"]] == list(th[:, fx.col("bonds")])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", rr.NAMES)
def test_oracle_rows_after_every_firing(name):
    """Fresh oracle runs up to every step at which the reference's bond or angle rows changed (every firing that did anything),
    and to the earlier checkpoint: rows as multisets, and at the checkpoint types, image flags, x and v."""
    fx = rr.fixture(name)
    steps = set(fx.change_steps()) | set(fx.checkpoints[:-1])
    if rr.has_angles(fx.scn):
        steps |= set(fx.change_steps("angle"))
    bad = []
    for step in sorted(steps - {0, fx.last}):
        got = rr.oracle_run(name, step)
        bad += rr.check_discrete(fx, step, got)
        if step in fx.checkpoints:
            bad += rr.check_continuous(fx, step, rr.deviation(fx, step, got["x"], got["image"], got["v"]), name)
    assert len(steps) >= 8
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# RanMars
# ------------------------------------------------------------------------------------------------------------------
def recorded_draws(seed):
    with np.load(os.path.join(rr.GOLDEN, "ref_ranmars.npz")) as z:
        return z["seed_%d" % seed].astype(np.int64)


@pytest.mark.parametrize("seed", rr.RANMARS_SEEDS)
def test_ranmars_streams(seed):
    """10008 uniform draws per seed, read out of the reference's Langevin forces on beads at rest, as 24-bit integers: the
    oracle's generator, the oracle's fix langevin run through the same script (draw k goes to bead k // 3 of the local order,
    component k % 3; every `run 0` draws another 3N), the host RanMarsInt from the start and after jump(k)."""
    from oracle import ranmars_stream
    from systems import run_oracle
    want = recorded_draws(seed)
    n = len(want)
    assert n == 3 * rr.RANMARS_BEADS * rr.RANMARS_RUNS and want.min() >= 0 and want.max() < 2 ** 24
    assert np.array_equal(ranmars_stream(seed, n) * 16777216.0, want)
    s = rr.ranmars_system()
    o = run_oracle(rr.ranmars_script(seed), s)
    f = []
    for _ in range(rr.RANMARS_RUNS):
        o.run(0)
        f.append(o.f())
    got, off = rr.draws_from_forces(np.concatenate(f))
    assert off < 1e-8 and np.array_equal(got, want)
    lib = ctypes.CDLL(os.path.join(ROOT, "lammps_le_amd", "liblammps_le.so"))
    fn = lib.lammps_le_test_ranmars
    fn.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    for skip in (0, 1, 96, 97, 98, 3336, 9000):
        out = np.zeros(1000)
        fn(seed, skip, 1000, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert np.array_equal(out * 16777216.0, want[skip:skip + 1000]), (seed, skip)


# ------------------------------------------------------------------------------------------------------------------
# the fixtures themselves
# ------------------------------------------------------------------------------------------------------------------
def test_fixture_conditions_and_sizes():
    """What the generator refuses to write, asked again of the committed files: (a) the count of FENE warnings is recorded (a run
    with an ERROR is never written), (b) the perturbed reruns left every row alone, (c) every fix acted (fix extrusion under
    respa: did not) and type-2 bonds exist, (d) the scenario's point was reached; the caps on beads, steps, periods and bytes."""
    meta = json.load(open(os.path.join(rr.GOLDEN, "ref_runs.json")))
    assert meta["build"]["packages"] == ["MOLECULE", "MC", "USER-LE"] and "-ffp-contract=off" in meta["build"]["cxx_flags"]
    assert sorted(meta["scenarios"]) == sorted(rr.NAMES)
    total = 0
    for fn in os.listdir(rr.GOLDEN):
        if fn.startswith("ref_"):
            size = os.path.getsize(os.path.join(rr.GOLDEN, fn))
            assert size < 2 ** 20, fn
            total += size
    assert total < 4 * 2 ** 20, total
    for name in rr.NAMES:
        fx = rr.fixture(name)
        m = fx.meta
        assert m["fene_warnings"] >= 0 and m["perturbed_reruns"] == 3 and m["perturbed_rows_identical"] is True, name
        assert rr.fixture_conditions(fx) == "", (name, rr.fixture_conditions(fx))
        assert fx.scn["system"]["n"] <= 2048 and fx.last <= 100 and m["steps"] == fx.last, name
        for ln in fx.scn["script"].split("\n"):
            w = ln.split()
            if w[:1] == ["fix"] and w[3] in ("extrusion", "ex_load", "ex_unload", "bond/create", "bond/break"):
                assert 4 <= int(w[4]) <= 10 and fx.last // int(w[4]) >= 4, ln
        # every spread the bounds come from is there and is a spread: positive after the first step
        assert all(fx.spread(q, c) > 0 for q in "xv" for c in fx.checkpoints) and fx.spread("f", fx.last) > 0, name
        assert np.asarray(fx.spread("thermo")).shape == fx.thermo()[:, 1:].shape, name
    # the rule the bounds rest on catches an FP32 intermediate (~1e-9 in x within 64 steps)
    assert all(rr.FACTOR * rr.fixture(n).spread("x", rr.fixture(n).last) < 1e-11 for n in rr.NAMES)


def test_data_files_are_the_recorded_ones(tmp_path):
    """The data file these tests write for a scenario is, byte for byte, the one the reference read (sha256)."""
    import hashlib
    from systems import write_data
    for name in rr.NAMES:
        fx = rr.fixture(name)
        path = os.path.join(str(tmp_path), "data.chain")
        write_data(path, fx.system())
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == fx.meta["data_sha256"], name


@pytest.mark.skipif(not os.path.isfile(LMP), reason="oracle/_ref/lmp is not built here (no reference tree)")
def test_regenerated_fixtures_are_the_committed_ones(tmp_path):
    """Two scenarios through the reference binary again: the fixture files and their entries of ref_runs.json, byte for byte."""
    import sys
    sys.path.insert(0, rr.GOLDEN)
    import make_reference_runs as gen
    committed = json.load(open(os.path.join(rr.GOLDEN, "ref_runs.json")))
    for name in ("roadblock_is_left", "newton_on_sort9"):
        scn = rr.BY_NAME[name]
        meta = gen.make_scenario(scn, str(tmp_path), rr.load_melt, out=str(tmp_path))
        new = open(os.path.join(str(tmp_path), "ref_%s.npz" % name), "rb").read()
        assert new == open(os.path.join(rr.GOLDEN, "ref_%s.npz" % name), "rb").read(), name
        assert json.loads(json.dumps(meta)) == committed["scenarios"][name], name
    # and one run that the reference aborts (test_reference_limits_cpu.py): error text, step and the state before it
    name = "limit_load_angles"
    meta = gen.make_limit(rr.LIMIT_BY_NAME[name], str(tmp_path), rr.load_melt, out=str(tmp_path))
    new = open(os.path.join(str(tmp_path), "ref_%s.npz" % name), "rb").read()
    assert new == open(os.path.join(rr.GOLDEN, "ref_%s.npz" % name), "rb").read(), name
    assert json.loads(json.dumps(meta)) == committed["limits"][name], name
