"""`minimize`, `min_style`, `min_modify`, fmax / fnorm without a GPU: the conditions on the recorded fixtures
(tests/minimize_runs.py), two fixtures regenerated where the reference binary exists, and the script layer's grammar and error
texts through the library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import minimize_runs as mn                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")


@pytest.mark.parametrize("name", mn.NAMES)
def test_fixture_conditions(name):
    fx = mn.fixture(name)
    assert mn.conditions(fx) == ""
    assert fx.z["thermo"].shape[1] == len(fx.columns)
    n = len(fx.z["x"])
    assert sorted(fx.z["local_order"]) == list(range(1, n + 1)) and fx.z["f"].shape == (n, 3) and fx.z["image"].shape == (n, 3)
    # the last row is the state that was dumped: fnorm and fmax of the recorded forces, to the rounding of the sums
    f = fx.z["f"].astype(np.longdouble)
    st = fx.stats()
    last = int(np.nonzero(fx.z["thermo"][:, 0] == st["iterations"])[0][0])      # (then_run: the rows of the run follow)
    assert abs(float(np.sqrt((f * f).sum())) - fx.z["thermo"][last, fx.col("fnorm")]) <= 1e-12 * max(1.0, fx.z["thermo"][last, fx.col("fnorm")])
    assert float(np.abs(fx.z["f"]).max()) == fx.z["thermo"][last, fx.col("fmax")]
    assert float("%.8g" % fx.z["thermo"][last, fx.col("fmax")]) == st["fmax_final"]
    assert float("%.8g" % fx.z["thermo"][0, fx.col("fmax")]) == st["fmax_initial"]
    assert float("%.15g" % fx.z["thermo"][last, fx.col("pe")]) == st["e_final"] and float("%.15g" % fx.z["thermo"][0, fx.col("pe")]) == st["e_initial"]


def test_stops_are_distinct():
    """Each stop scenario ends with its own index, strictly before maxiter; the two line searches differ in evaluations."""
    stops = {n: int(mn.fixture(n).stats()["stop"]) for n in mn.NAMES}
    assert stops["stop_etol"] == mn.ETOL and stops["stop_maxeval"] == mn.MAXEVAL and stops["stop_zeroforce"] == mn.DOWNHILL
    assert stops["stop_ftol_two"] == stops["stop_ftol_max"] == stops["stop_ftol_inf"] == mn.FTOL
    its = {n: int(mn.fixture(n).stats()["iterations"]) for n in ("stop_ftol_two", "stop_ftol_max", "stop_ftol_inf")}
    assert len(set(its.values())) > 1, its          # (the three norms do not all stop on the same iteration)
    assert mn.fixture("cg_default").stats()["evals"] != mn.fixture("sd_backtrack").stats()["evals"]
    a, b = mn.fixture("cg_default").z["thermo"], mn.fixture("norm_no").z["thermo"]
    assert np.allclose(b[0, 2], a[0, 2] * mn.N, rtol=1e-14) and not np.array_equal(a[:, 0], []) and a.shape == b.shape


@pytest.mark.skipif(not os.path.isfile(LMP), reason="the reference binary is not built here")
@pytest.mark.parametrize("name", ["stop_maxeval", "dmax_small", "crossing"])
def test_fixture_regenerates(name, tmp_path):
    import make_minimize_runs as mk
    assert mk.main([name], out=str(tmp_path)) == 0
    with np.load(os.path.join(str(tmp_path), "minimize_%s.npz" % name)) as z:
        for k in z.files:
            assert np.array_equal(z[k], mn.fixture(name).z[k]), k


# ------------------------------------------------------------------------------------------------------------------
# the long-double restatement (minimize_reference.py) through every fixture
# ------------------------------------------------------------------------------------------------------------------
_restated = {}


def restated(name):
    import minimize_reference as mref
    if name not in _restated:
        fx = mn.fixture(name)
        _restated[name] = mref.run(fx.scn, mn.system(fx.scn))
    return _restated[name]


SUM_ROUNDINGS = 64


@pytest.mark.parametrize("name", mn.NAMES)
def test_restatement_against_fixture(name):
    """The algorithm in long double over the brute-force forces gives the recorded iteration count, evaluation count, stop
    index, list builds and image flags exactly, and the final x under 16 x the recorded spread.  The thermo rows: a cell's
    three-rerun spread is 0 or 1 ulp of the value in many cells (three draws of a sum that lands 0 to 6 ulps apart), and the
    restatement - the exact value - lies up to 23 such spreads from the record, so the rows are held to 16 x the larger of the
    spread and SUM_ROUNDINGS roundings of the value: pe, emol and fnorm are sums of 1000 to 3000 terms of one sign or of
    cancelling signs many times the result, added one after another in double by the program that was recorded; sqrt(3000)
    is 55 roundings, the typical error of such a sum.  The distances are printed."""
    import minimize_reference as mref
    fx, r, st = mn.fixture(name), restated(name), mn.fixture(name).stats()
    assert (r["iterations"], r["evals"], r["stop"], r["builds"]) == (int(st["iterations"]), int(st["evals"]), int(st["stop"]), int(fx.z["builds"][0]))
    assert np.array_equal(r["image"], fx.z["image"])
    assert float("%.8g" % r["alpha"]) == st["alpha"] or abs(r["alpha"] - st["alpha"]) <= 1e-7 * st["alpha"]
    dx, sx = float(np.abs(r["x"] - fx.z["x"]).max()), fx.meta["spread"]["x"]
    assert dx <= mn.FACTOR * sx, (dx, sx)
    cols = mref.columns(fx.scn)
    th = fx.z["thermo"][:len(r["rows"])]
    assert np.array_equal(th[:, 0], r["rows"][:, 0])
    sp = np.asarray(fx.meta["spread"]["thermo"])[:len(th)]
    worst_spread, worst = 0.0, 0.0
    for k, nm in enumerate(cols):
        c = fx.col(nm)
        for row in range(len(th)):
            d = abs(r["rows"][row, k + 1] - th[row, c])
            b = mn.FACTOR * max(sp[row, c - 1], SUM_ROUNDINGS * 2.220446049250313e-16 * abs(th[row, c]))
            worst = max(worst, d / b if b > 0 else (0.0 if d == 0 else np.inf))
            if sp[row, c - 1] > 0:
                worst_spread = max(worst_spread, d / sp[row, c - 1])
            assert d <= b, (nm, row, d, b)
    print("%-18s x %.2e (spread %.2e); rows at most %.2f of their bound, %.1f spreads where the spread is not 0" % (name, dx, sx, worst, worst_spread))


def test_line_search_exits():
    """Which exit the line searches take, read off the restatement: cg_default leaves all 30 through the quadratic projection
    (the melt never needs to backtrack under the quadratic search), sd_backtrack all through the backtracking exit, and
    dmax_small and soft_overlap take the first trial, at alphamax, in most iterations and the projection in the others."""
    from collections import Counter
    ex = {n: Counter(restated(n)["exits"]) for n in ("cg_default", "sd_backtrack", "dmax_small", "soft_overlap")}
    assert ex["cg_default"] == {"quadratic": 30}
    assert ex["sd_backtrack"] == {"backtrack": 30}
    assert ex["dmax_small"]["alphamax"] >= 1 and ex["dmax_small"]["quadratic"] >= 1
    assert ex["soft_overlap"]["alphamax"] >= 1 and ex["soft_overlap"]["quadratic"] >= 1


# ------------------------------------------------------------------------------------------------------------------
# grammar and error texts through the library (no device is touched before a minimisation starts)
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def handle(tmp_path):
    from lammps_le_amd import lammps
    from systems import write_data
    scn = mn.BY_NAME["cg_default"]
    data = os.path.join(str(tmp_path), "data.chain")
    write_data(data, mn.system(scn))
    p = lammps(cmdargs=["-screen", "none"])
    p.head = [ln.replace("read_data data.chain", "read_data " + data) for ln in scn["head"].split("\n")]
    yield p
    p.close()


def refused(p, cmd, text):
    with pytest.raises(Exception) as e:
        p.command(cmd)
    assert text in str(e.value), (cmd, str(e.value))


def test_before_box(handle):
    refused(handle, "minimize 0 0 10 10", "Minimize command before simulation box is defined")
    refused(handle, "min_style cg", "Min_style command before simulation box is defined")
    refused(handle, "minimize 0 0 10", "Illegal minimize command")


def test_grammar(handle):
    p = handle
    for ln in p.head:
        p.command(ln)
    refused(p, "minimize 0 0 10", "Illegal minimize command")
    refused(p, "minimize 0 0 10 10 10", "Illegal minimize command")
    refused(p, "minimize -1.0 0 10 10", "Illegal minimize command")
    refused(p, "minimize 0 -1.0 10 10", "Illegal minimize command")
    for style in ("fire", "fire/old", "quickmin", "hftn", "spin", "spin/cg", "spin/lbfgs"):
        refused(p, "min_style " + style, "MI355X engine: min_style %s is not on the device" % style)
    refused(p, "min_style bogus", "Illegal minimize style")
    p.command("min_style sd")
    p.command("min_style cg")
    refused(p, "min_modify", "Illegal min_modify command")
    refused(p, "min_modify dmax", "Illegal min_modify command")
    refused(p, "min_modify line bogus", "Illegal min_modify command")
    refused(p, "min_modify norm bogus", "Illegal min_modify command")
    refused(p, "min_modify halfstepback maybe", "Illegal min_modify command")
    refused(p, "min_modify integrator bogus", "Illegal min_modify command")
    refused(p, "min_modify bogus 1", "Illegal fix_modify command")          # (the reference's words, src/min.cpp:747)
    for line in ("forcezero", "spin_cubic", "spin_none"):
        refused(p, "min_modify line " + line, "MI355X engine: min_modify line %s is not on the device" % line)
    p.command("min_modify dmax 0.05 line backtrack norm max")
    p.command("min_modify line quadratic norm inf")
    p.command("min_modify norm two delaystep 5 dtgrow 1.1 dtshrink 0.5 alpha0 0.1 alphashrink 0.9 tmax 10 tmin 0.02 vdfmax 100")
    p.command("min_modify halfstepback yes initialdelay no integrator verlet")


def test_fmax_fnorm_keywords(handle):
    p = handle
    for ln in p.head:
        p.command(ln)
    p.command("thermo_style custom step pe fmax fnorm")
    p.command("variable a equal fmax")
    p.command("variable b equal fnorm*2")
    assert p.get_thermo("fmax") == 0.0 and p.get_thermo("fnorm") == 0.0          # (nothing evaluated yet)
    refused(p, "thermo_style custom step fmaxx", "Unknown keyword in thermo_style custom command")
    p.command("thermo_modify format float %.17g")
    refused(p, "thermo_modify format float %s", "MI355X engine: thermo_modify format float")


def test_python_method_exists():
    from lammps_le_amd import lammps
    assert callable(getattr(lammps, "minimize"))
