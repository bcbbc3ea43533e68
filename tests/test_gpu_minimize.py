"""`minimize` on the device against the recorded reference minimisations (tests/minimize_runs.py, tests/golden/minimize_*.npz).

Exact: iteration count, evaluation count, stop index, list builds, bond rows, image flags, local order at the end, the step
the handle is left on.  Thermo rows (with fmax / fnorm), final x and f and the numbers of the stats block: under 16 x the
reference's own spread over its three reruns from starts moved by one ulp (the project's standing rule; the device's reductions
add in another order, which perturbs at that scale).  There is no floor under the spread.  An energy or a force norm is a sum
of a few thousand terms whose three reruns land 0 to 6 ulps of the value apart, so a cell's spread of 0 or 1 ulp is a
coincidence of three draws: the long-double restatement of the same minimisation (tests/minimize_reference.py), which is the
exact value of every such cell, lies up to 23 spreads from the recorded row (test_minimize_cpu.py prints the figures).  For
the cells the restatement holds (pe, epair, emol, eangle, fmax, fnorm, the fixes' energies) the bound is therefore 16 x the larger of
the spread and the recorded value's own distance from the restatement - the reference's own error, measured, never the
engine's.  Measured on an MI355X: every thermo cell at most 0.19 of its bound (the figures per scenario are in README).  Two kinds of cell cannot spread at all and
are held otherwise: temp - the reruns move coordinates and leave every velocity alone, so its spread is 0 by construction; the
minimiser never changes a velocity either, so temp is compared with the long-double value from the start's velocities, within
TEMP_ROUNDINGS roundings (3 N = 3000 positive products added in a tree of blocks: a thread's three, six shuffle levels, four
wavefronts, the column sum's rows - under 32 additions deep, each within half an ulp of a sum that only grows) - and any cell
whose three reruns agree to the last bit (the zero forces under `setforce 0 0 0`), which must be met exactly.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import minimize_reference as mref               # noqa: E402
import minimize_runs as mn                      # noqa: E402
import reference_runs as rr                     # noqa: E402

pytestmark = pytest.mark.gpu
TEMP_ROUNDINGS = 32
EPS = 2.220446049250313e-16

_runs = {}


def run(name, tmp_path_factory):
    if name not in _runs:
        _runs[name] = mn.run_engine(mn.BY_NAME[name], tmp_path_factory.mktemp("min_" + name))
    return _runs[name]


def bound(spread):
    """16 x the reference's own spread; a cell the reruns agree on to the last bit is met exactly."""
    return mn.FACTOR * spread


_exact = {}


def exact_rows(fx):
    """The rows of the minimisation from the long-double restatement (minimize_reference.py), by column name."""
    if fx.name not in _exact:
        r = mref.run(fx.scn, mn.system(fx.scn))
        _exact[fx.name] = {nm: r["rows"][:, k + 1] for k, nm in enumerate(mref.columns(fx.scn))}
    return _exact[fx.name]


def cell(fx, rows, th, sp, r, c, temp):
    """(distance, bound) of one thermo cell against the record: 16 x the larger of the spread of the reference's three reruns
    and the recorded value's own distance from the long-double restatement of the same minimisation (the reference's own
    error: where the restatement holds the cell).  temp while no velocity has changed against its long-double value."""
    name = fx.columns[c]
    if name == "temp" and sp[r, c - 1] == 0.0:
        return abs(rows[r, c] - temp), TEMP_ROUNDINGS * EPS * temp
    own = 0.0
    ex = exact_rows(fx)
    if name in ex and r < len(ex[name]):          # (then_run: the rows of the run lie behind the restatement's)
        own = abs(th[r, c] - ex[name][r])
    return abs(rows[r, c] - th[r, c]), bound(max(sp[r, c - 1], own))


def temp_of(system):
    """compute temp (src/compute_temp.cpp) of the start's velocities in long double, lj units."""
    v = np.asarray(system["v"], dtype=np.longdouble)
    m = np.asarray([system["mass"][t - 1] for t in system["type"]], dtype=np.longdouble)
    return float((m[:, None] * v * v).sum() / (3 * len(v) - 3))


@pytest.mark.parametrize("name", mn.NAMES)
def test_scenario(name, tmp_path_factory):
    fx, got = mn.fixture(name), run(name, tmp_path_factory)
    st, mine = fx.stats(), got["stats"]
    # exact
    assert (mine["iterations"], mine["evals"], mine["stop"], mine["steps"]) == (int(st["iterations"]), int(st["evals"]), int(st["stop"]), int(st["steps"]))
    assert (int(got["stat"]["min_iterations"]), int(got["stat"]["min_evals"]), int(got["stat"]["min_stop"])) == (mine["iterations"], mine["evals"], mine["stop"])
    assert mine["builds"] == [int(b) for b in fx.z["builds"]][:1]
    assert int(got["stat"]["min_rebuilds"]) == mine["builds"][-1]
    assert mine["warned"]
    assert got["step"] == int(st["iterations"])
    assert np.array_equal(got["image"], fx.z["image"])
    assert np.array_equal(got["local_order"], fx.z["local_order"])
    s = mn.system(fx.scn)
    assert np.array_equal(got["bonds"], rr.sort_rows(np.asarray(s["bonds"], dtype=np.int64)))
    # thermo rows, x, f, stats under 16 x the reference's spread
    th, sp = fx.z["thermo"], np.asarray(fx.meta["spread"]["thermo"])
    if fx.scn["after"]:          # (then_run: the rows of the run follow, test_then_run_record)
        th = th[:len(got["thermo"])]
        assert th[-1, 0] == st["iterations"]
    assert got["thermo"].shape == th.shape and np.array_equal(got["thermo"][:, 0], th[:, 0])
    bad, worst, temp = [], 0.0, temp_of(s)
    for r in range(th.shape[0]):
        for c in range(1, th.shape[1]):
            err, b = cell(fx, got["thermo"], th, sp, r, c, temp)
            worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
            if not err <= b:
                bad.append("row %d %s: %.3e exceeds %.3e" % (r, fx.columns[c], err, b))
    dx = float(np.abs(got["x"] - fx.z["x"]).max())
    df = float(np.abs(got["f"] - fx.z["f"]).max())
    bx, bf = bound(fx.meta["spread"]["x"]), bound(fx.meta["spread"]["f"])
    print("%-18s thermo %.2f of its bound; x %.2e (bound %.2e); f %.2e (bound %.2e)" % (name, worst, dx, bx, df, bf))
    if not dx <= bx:
        bad.append("x: %.3e exceeds %.3e" % (dx, bx))
    if not df <= bf:
        bad.append("f: %.3e exceeds %.3e" % (df, bf))
    # the stats block: the printed numbers ({:18.15g} and {:.8}) to the digits the spread leaves stable
    for k in ("e_initial", "e_previous", "e_final", "fnorm_initial", "fnorm_final", "fmax_initial", "fmax_final", "alpha", "max_move"):
        digits = 15 if k.startswith("e_") else 8
        b = max(bound(fx.meta["spread"]["stats"][k]), 10.0 ** (-digits + 1) * abs(st[k]))          # (one unit of the last printed digit)
        if not abs(mine[k] - st[k]) <= b:
            bad.append("stats %s: %.17g against %.17g (bound %.3e)" % (k, mine[k], st[k], b))
    # last_thermo is the last row
    assert got["pe"] == got["thermo"][-1, fx.col("pe")] and got["fmax"] == got["thermo"][-1, fx.col("fmax")]
    assert got["fnorm"] == got["thermo"][-1, fx.col("fnorm")]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", mn.NAMES)
def test_wait_budget_and_downloads(name, tmp_path_factory):
    """One wait per evaluation, one per rebuild, one per direction update, plus set-up; nothing downloaded."""
    s = run(name, tmp_path_factory)["stat"]
    assert s["min_host_waits"] <= s["min_evals"] + s["min_rebuilds"] + s["min_iterations"] + 8, s
    assert s["host_downloads"] == 0, s


@pytest.mark.parametrize("name", ["cg_default", "confined_tethered", "angles", "soft_overlap"])
def test_end_state_against_brute_force(name, tmp_path_factory):
    """Independent of the reference's trajectory: forces and pe at the gathered end positions against the long-double brute
    force - force_reference.py, with soft_reference.py for the soft pair term and wall_reference.py / extforce_reference.py
    for the walls and the force fixes -, within the bound test_gpu_force.py holds single evaluations to."""
    import force_reference as fr
    from force_compare import RUN0_CEILING, relerr
    fx, got = mn.fixture(name), run(name, tmp_path_factory)
    s = mn.system(fx.scn)
    text = fx.scn["head"] + "run 0\n"          # (styles and coefficients; the fixes of `before` are restated below)
    if name == "soft_overlap":
        import soft_reference as sr
        model = fr.model_from_script(text.replace("pair_style soft 1.12246\npair_coeff * * 30.0\n", "pair_style zero 1.12246\n"), s["ntypes"])
        model.pair = sr.soft_model_pair(1.12246, [(1, 1, 30.0)])
        S = sr.SoftSystem(model, s["box"], s["type"], s["mass"], s["bonds"])
    else:
        S = fr.System(fr.model_from_script(text, s["ntypes"]), s["box"], s["type"], s["mass"], s["bonds"], s.get("angles"))
    box = np.asarray(s["box"], dtype=np.float64)
    x = got["x"]          # (between two list builds a bead may sit just outside the box: wrapped for the brute force)
    ev = S.evaluate(box[:, 0] + np.mod(x - box[:, 0], box[:, 1] - box[:, 0]))
    want_f, efix = ev.f, 0
    if name == "confined_tethered":
        want_f, e = mref.confined_fixes(fx.scn, s, x, got["image"], ev.f, got["step"])          # (step 24: the addforce acts)
        efix = e["f_w"] + e["f_s"] + e["f_a"]
    ef = relerr(got["f"], want_f)
    pe = float((ev.evdwl + ev.ebond + ev.eangle + efix) / len(x))
    ee = abs(got["pe"] - pe) / max(abs(pe), 1.0)
    print("%s end state: forces %.2e, pe %.2e off the brute force" % (name, ef, ee))
    assert ef <= RUN0_CEILING and ee <= RUN0_CEILING


def test_energy_never_rises(tmp_path_factory):
    for name in ("cg_default", "confined_tethered", "angles"):
        pe = run(name, tmp_path_factory)["thermo"][:, mn.COLUMNS.index("pe")]
        assert (np.diff(pe) <= 0).all(), (name, pe)


def test_repeatable(tmp_path_factory):
    """The same minimisation twice on fresh handles: x, f and thermo bit for bit."""
    a = run("cg_default", tmp_path_factory)
    b = mn.run_engine(mn.BY_NAME["cg_default"], tmp_path_factory.mktemp("again"))
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["f"], b["f"]) and np.array_equal(a["thermo"], b["thermo"])


def test_zero_alpha_restores_start(tmp_path_factory):
    """stop_zeroforce: nothing moves - the positions after the minimisation are the start, bit for bit."""
    got = run("stop_zeroforce", tmp_path_factory)
    assert np.array_equal(got["x"], mn.system(mn.BY_NAME["stop_zeroforce"])["x"])


def test_then_run_continues_and_cleans_up(tmp_path_factory):
    """A run after a minimisation continues the step count on the fused path with the script's neighbour settings; the
    minimiser's vectors are gone from the device; minimize() returns the stats block."""
    from lammps_le_amd import lammps
    from systems import write_data
    scn = mn.BY_NAME["stop_etol"]
    tmp = tmp_path_factory.mktemp("then_run")
    write_data(os.path.join(str(tmp), "data.chain"), mn.system(scn))
    p = lammps(cmdargs=["-screen", "none"])
    try:
        for ln in mn.script(scn).split("\n"):
            if ln.startswith("minimize"):
                break
            p.command(ln.replace("read_data data.chain", "read_data " + os.path.join(str(tmp), "data.chain")))
        p.command("fix 1 all nve")
        p.command("fix 2 all langevin 1.0 1.0 1.0 904297")
        p.command("run 0")
        before = p.stat("device_bytes")
        out = p.minimize(*mn.minimize_args(scn))
        assert p.stat("device_bytes") == before
        st = mn.fixture("stop_etol").stats()
        assert out["stop"] == mn.STOP_STRINGS[int(st["stop"])] and out["iterations"] == int(st["iterations"]) and out["evals"] == int(st["evals"])
        assert out["e_final"] == p.get_thermo("pe") and out["fnorm"] == p.get_thermo("fnorm") and out["alpha"] == p.stat("min_alpha")
        p.command("run 20")
        assert int(p.get_thermo("step")) == int(st["iterations"]) + 20
        assert p.stat("steps_fused") > 0
    finally:
        p.close()


def test_refusals(tmp_path_factory):
    """min_style fire, min_modify line forcezero and the illegal forms: the error text, and the handle still works."""
    from lammps_le_amd import lammps
    from systems import write_data
    scn = mn.BY_NAME["cg_default"]
    tmp = tmp_path_factory.mktemp("refuse")
    data = os.path.join(str(tmp), "data.chain")
    write_data(data, mn.system(scn))
    p = lammps(cmdargs=["-screen", "none"])
    try:
        for ln in scn["head"].split("\n"):
            p.command(ln.replace("read_data data.chain", "read_data " + data))
        for cmd, text in (("min_style fire", "MI355X engine: min_style fire is not on the device"),
                          ("min_modify line forcezero", "MI355X engine: min_modify line forcezero is not on the device"),
                          ("min_style bogus", "Illegal minimize style"), ("minimize 0 0 10", "Illegal minimize command"),
                          ("minimize -1 0 10 10", "Illegal minimize command"), ("min_modify dmax", "Illegal min_modify command")):
            with pytest.raises(Exception, match=text):
                p.command(cmd)
        p.command("minimize 0 0 3 100")
        assert int(p.stat("min_iterations")) == 3
    finally:
        p.close()


def test_repeatable_after_md_and_read_restart(tmp_path_factory):
    """A handle writes a restart file of the start and runs 50 MD steps; the start read back with read_restart gives
    cg_default's x, f and thermo bit for bit.  (read_restart needs a handle without a box and the engine refuses `clear`, so
    the file is read by a second handle.)"""
    from lammps_le_amd import lammps
    from systems import write_data
    scn = mn.BY_NAME["cg_default"]
    a = run("cg_default", tmp_path_factory)
    tmp = str(tmp_path_factory.mktemp("restart"))
    data, rst, log = (os.path.join(tmp, n) for n in ("data.chain", "start.restart", "log.min"))
    write_data(data, mn.system(scn))
    lines = [ln.replace("read_data data.chain", "read_data " + data) for ln in mn.script(scn).split("\n")]
    k = next(i for i, ln in enumerate(lines) if ln.startswith("thermo_style"))
    p = lammps(cmdargs=["-screen", "none"])
    try:
        for ln in lines[:k] + ["write_restart " + rst, "fix 1 all nve", "fix 2 all langevin 1.0 1.0 1.0 904297", "run 50"]:
            p.command(ln)
        assert int(p.get_thermo("step")) == 50
    finally:
        p.close()
    p = lammps(cmdargs=["-screen", "none", "-log", log])
    try:
        # (as in the reference, styles and settings are given again around read_restart; the file holds the atoms and the box)
        for ln in lines:
            p.command("read_restart " + rst if ln.startswith("read_data") else ln)
        x, f = p.gather("x"), p.gather("f")
    finally:
        p.close()
    rows, st = mn.parse_log(open(log).read(), len(mn.columns(scn)))
    assert np.array_equal(x, a["x"]) and np.array_equal(f, a["f"]) and np.array_equal(rows, a["thermo"])
    assert st["iterations"] == a["stats"]["iterations"] and st["evals"] == a["stats"]["evals"]


def test_nothing_left_allocated(tmp_path_factory):
    """After close() nothing of a handle that minimised is left: device blocks, pinned blocks, streams and events."""
    from test_gpu_devmem import live
    before = live()
    got = mn.run_engine(mn.BY_NAME["stop_maxeval"], tmp_path_factory.mktemp("alloc"))
    assert got["stats"]["iterations"] > 0
    assert live() == before


def test_two_slabs_fmax_fnorm_and_refusal(tmp_path):
    """fmax / fnorm on a decomposed MD run: the maximum exactly, the norm to the rounding of its sum, against the gathered
    forces, and both against one GPU as the other slab tests compare; `minimize` is refused on every rank with the engine's
    text and the handle runs on."""
    import pickle
    import subprocess
    import uuid

    import extforce_runs as ex
    from dd_minimize_worker import results
    from systems import run_product
    system = ex.fixture("crossing").system()
    script = rr._DD + "thermo_style custom step pe fmax fnorm\nthermo 10\nrun 30\n"
    p = run_product(script, system, tmp_path)
    one = results(p)
    p.close()
    session = uuid.uuid4().hex[:12]
    here = os.path.dirname(os.path.abspath(__file__))
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out.npz"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "dd_minimize_worker.py"), str(r), "2", session, sysfile, scriptfile, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    assert all(q.returncode == 0 for q in procs), "\n".join(logs)
    r = np.load(out)
    assert r["nranks"][0] == 2 and 0 < r["nlocal"][0] < len(system["x"])
    for res in (one, r):
        f = np.asarray(res["f"], dtype=np.longdouble)
        assert res["fmax"][0] == float(np.abs(res["f"]).max()) and res["fmax"][0] > 0
        assert abs(res["fnorm"][0] - float(np.sqrt((f * f).sum()))) <= 64 * EPS * res["fnorm"][0]
    assert abs(r["fmax"][0] - one["fmax"][0]) <= 1e-9 * one["fmax"][0] and abs(r["fnorm"][0] - one["fnorm"][0]) <= 1e-9 * one["fnorm"][0]
    assert "MI355X engine: minimize is not supported on a decomposed handle" in str(r["refusal"][0])
    assert int(r["step"][0]) == 35 and r["fmax_after"][0] == float(np.abs(r["f_after"]).max())


def test_then_run_record(tmp_path_factory):
    """then_run: the 24 MD steps behind the minimisation against the record - step count continued, local order (an Atom::sort
    fell inside the minimisation), image flags, bond rows and the LE fixes' counters exactly, x and v and the run's thermo rows
    under 16 x the reference's spread, on the fused path."""
    fx, got = mn.fixture("then_run"), run("then_run", tmp_path_factory)
    a, z = got["after"], fx.z
    it = int(fx.stats()["iterations"])
    assert a["step"] == it + mn.THEN_RUN and a["steps_fused"] > 0
    assert np.array_equal(got["bonds"], rr.sort_rows(z["bond_rows_min"].astype(np.int64)))
    assert np.array_equal(a["bonds"], rr.sort_rows(z["bond_rows_after"].astype(np.int64))) and not np.array_equal(a["bonds"], got["bonds"])
    assert np.array_equal(a["local_order"], z["local_order_after"]) and np.array_equal(a["image"], z["image_after"])
    th, sp = z["thermo"], np.asarray(fx.meta["spread"]["thermo"])
    assert a["thermo"].shape == th.shape and np.array_equal(a["thermo"][:, 0], th[:, 0])
    for f in rr.LE3:
        assert a["fixvec"][f] == (th[-1, fx.col("f_%s[1]" % f)], th[-1, fx.col("f_%s[2]" % f)]), f
    s = mn.system(fx.scn)
    L = (np.asarray(s["box"])[:, 1] - np.asarray(s["box"])[:, 0])[None, :]
    dx = float(np.abs((a["x"] + a["image"] * L) - (z["x_after"] + z["image_after"] * L)).max())
    dv = float(np.abs(a["v"] - z["v_after"]).max())
    bad, worst = [], 0.0
    first_run_row = len(got["thermo"])
    for r in range(first_run_row, th.shape[0]):
        for c in range(1, th.shape[1]):
            err, b = cell(fx, a["thermo"], th, sp, r, c, temp_of(s))
            worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
            if not err <= b:
                bad.append("row %d %s: %.3e exceeds %.3e" % (r, fx.columns[c], err, b))
    bx, bv = bound(fx.meta["spread"]["x_after"]), bound(fx.meta["spread"]["v_after"])
    print("then_run after the run: thermo %.2f of its bound; x %.2e (bound %.2e); v %.2e (bound %.2e)" % (worst, dx, bx, dv, bv))
    assert dx <= bx and dv <= bv and not bad, "\n".join(bad)
