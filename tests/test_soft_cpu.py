"""pair_style soft, fix adapt and ramp() without a device: the long-double soft term (soft_reference.py) against the reference
program's own known answers, the inline sine / cosine / pair term of soft_inl.h compiled for the host against long double,
the step plan with soft requests against the instantiations of the step kernel, the script layer through the C-ABI and the
host-side coefficient hook, and the conditions the recorded fixtures were made under (soft_runs.py)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import force_compare as fc
import force_reference as fr
import soft_reference as sr
import soft_runs as so
from neigh_reference import LD
from systems import CHAIN_SCRIPT, lattice_chain, write_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PD = ctypes.POINTER(ctypes.c_double)


def _lib():
    from lammps_le_amd import library_path
    return ctypes.CDLL(library_path())


# ------------------------------------------------------------------------------------------------------------------
# 1. the reference program's known answers
# ------------------------------------------------------------------------------------------------------------------
def test_soft_reference_reproduces_known_answers():
    """Initial energy, forces and stress of data.fourmol under pair_style soft 8.0 (six pair_coeff rows with their own rc, the
    rest mixed: A geometric, rc arithmetic) within the fixture's own epsilon of 5e-14, by the rule
    test_force_reference_cpu.py uses for lj_cut (energy relative, forces and stress relative with floor 1).
    Measured: energy 6.7e-16, forces 9.4e-17, stress 2.0e-16."""
    d = json.load(open(os.path.join(G, "fourmol.json")))
    g = json.load(open(os.path.join(G, "pair_soft.json")))
    assert g["epsilon"] == 5e-14 and g["pair_style"] == "soft"
    order = np.argsort(np.array(d["tag"]))
    m = fr.Model()
    m.units, m.special_lj = "real", tuple(d["special_lj"])
    m.pair = sr.soft_model_pair(g["cut_global"], [(int(r[0]), int(r[1]), r[2], r[3]) for r in g["pair_coeff"]], mix=g["mix"])
    S = sr.SoftSystem(m, d["box"], np.array(d["type"])[order], [d["mass"][str(t + 1)] for t in range(d["ntypes"])], d["bonds"], d["angles"])
    ev = S.evaluate(np.array(d["x"])[order])
    de = float(abs(ev.evdwl - LD(g["init_energy"])) / abs(LD(g["init_energy"])))
    df, dv = fc.relerr(ev.f, g["init_forces"]), fc.relerr(ev.vpair, g["init_stress"])
    print("pair_soft: energy %.2e forces %.2e stress %.2e (epsilon %.1e)" % (de, df, dv, g["epsilon"]))
    assert de < g["epsilon"] and df < g["epsilon"] and dv < g["epsilon"]
    assert ev.ebond == 0 and len(ev.terms["pair"][0]) >= 50          # (70 interacting pairs)


# ------------------------------------------------------------------------------------------------------------------
# 2. the inline sine and the pair term
# ------------------------------------------------------------------------------------------------------------------
RCS = (1.0, 1.12246, 2.5)
A_TEST = 60.0


def pair_points(rc):
    """rsq of: r = 0, the smallest positive rsq, r one ulp below rc, both sides of the fold at rc / 2, 10^5 random r in (0, rc);
    all with rsq < rc * rc as the kernel's cutoff test sees it"""
    rng = np.random.RandomState(int(rc * 1000))
    r = [0.0]
    below = np.nextafter(rc, 0.0)
    while below * below >= rc * rc:
        below = np.nextafter(below, 0.0)
    half = 0.5 * rc
    fold = [half]
    for k in range(4):
        fold += [np.nextafter(fold[-1], np.inf)]
    lo = half
    for k in range(4):
        lo = np.nextafter(lo, 0.0)
        fold.append(lo)
    r += [below] + fold + list(rng.uniform(0.0, rc, size=100000))
    rsq = np.array(r) ** 2
    rsq[0] = 0.0
    rsq = np.concatenate([rsq, [5e-324]])
    assert (rsq < rc * rc).all() and rsq[-1] > 0
    return rsq


def test_inline_pair_term_against_long_double():
    """fpair and the energy of soft_inl.h's pair term (host build, the same fma's the kernels run) against long double.
    Metric: |fpair - ref| r / (A pi / rc) - the error of the force in units of the largest force the pair can exert - and
    |E - ref| / A.  Bound: 4 x the same figure of a float64 restatement of PairSoft::compute's own operation order
    (sqrt, MY_PI * r / rc, the library's sin and cos, the products left to right), measured here over the same points - it comes
    from the reference's arithmetic, not from the code under test; the factor 4 is one step of headroom for a polynomial against
    a correctly rounded library.  Coincident beads: zero force, energy 2 A, nothing non-finite.
    Measured (max over rc = 1.0, 1.12246, 2.5): force 5.1e-16 against the restatement's 6.8e-16, energy 4.1e-16 against 5.8e-16;
    the sine alone on [0, pi]: 2.0e-16 absolute (numpy: 5.6e-17)."""
    lib = _lib()
    worst = dict(f=0.0, e=0.0, f_ref=0.0, e_ref=0.0)
    for rc in RCS:
        rsq = pair_points(rc)
        f, e = np.zeros_like(rsq), np.zeros_like(rsq)
        lib.lammps_le_test_soft_pair(len(rsq), rsq.ctypes.data_as(PD), ctypes.c_double(A_TEST), ctypes.c_double(rc), f.ctypes.data_as(PD),
                                     e.ctypes.data_as(PD))
        assert np.isfinite(f).all() and np.isfinite(e).all()
        assert f[0] == 0.0 and e[0] == 2.0 * A_TEST                    # r = 0: no 0 * inf
        # long double, from the same rsq
        r = np.sqrt(rsq.astype(LD))
        arg = fr.PI * r / LD(rc)
        safe = np.where(r > 0, r, LD(1))
        f_ld = np.where(r > 0, LD(A_TEST) * np.sin(arg) * fr.PI / LD(rc) / safe, LD(0))
        e_ld = LD(A_TEST) * (1 + np.cos(arg))
        # float64 in the reference's operation order (pair_soft.cpp:97-113)
        r64 = np.sqrt(rsq)
        arg64 = np.pi * r64 / rc
        with np.errstate(invalid="ignore", divide="ignore"):
            f64 = np.where(r64 > 0, 1.0 * A_TEST * np.sin(arg64) * np.pi / rc / r64, 0.0)
        e64 = 1.0 * A_TEST * (1.0 + np.cos(arg64))
        scale = r / (LD(A_TEST) * fr.PI / LD(rc))
        worst["f"] = max(worst["f"], float((np.abs(f - f_ld) * scale).max()))
        worst["f_ref"] = max(worst["f_ref"], float((np.abs(f64 - f_ld) * scale).max()))
        worst["e"] = max(worst["e"], float((np.abs(e - e_ld) / A_TEST).max()))
        worst["e_ref"] = max(worst["e_ref"], float((np.abs(e64 - e_ld) / A_TEST).max()))
        # the smallest positive rsq: the force factor tends to A (pi / rc)^2 and must be right RELATIVE to it
        assert abs(f[-1] / float(f_ld[-1]) - 1.0) < 1e-15
    print("pair term: force %.2e (restatement %.2e), energy %.2e (restatement %.2e)" % (worst["f"], worst["f_ref"], worst["e"], worst["e_ref"]))
    assert worst["f_ref"] > 0 and worst["e_ref"] > 0
    assert worst["f"] <= 4.0 * worst["f_ref"], worst
    assert worst["e"] <= 4.0 * worst["e_ref"], worst


def test_inline_sine_on_its_range():
    """sin and cos of soft_inl.h on [0, pi]: 10^5 points, the ends, and the doubles around the fold at pi / 2; bound as above,
    4 x the library's own error over the same points (at least half an ulp of 1)."""
    lib = _lib()
    x = np.concatenate([np.linspace(0.0, np.pi, 100001), np.pi / 2 + np.arange(-6, 7) * 2.2e-16, np.random.RandomState(3).uniform(0, np.pi, 100000)])
    x = x[x <= np.pi]
    s, c = np.zeros_like(x), np.zeros_like(x)
    lib.lammps_le_test_soft_sincos(len(x), x.ctypes.data_as(PD), s.ctypes.data_as(PD), c.ctypes.data_as(PD))
    xl = x.astype(LD)
    es, ec = float(np.abs(s - np.sin(xl)).max()), float(np.abs(c - np.cos(xl)).max())
    ns, nc = float(np.abs(np.sin(x) - np.sin(xl)).max()), float(np.abs(np.cos(x) - np.cos(xl)).max())
    print("sin %.2e (library %.2e)  cos %.2e (library %.2e)" % (es, ns, ec, nc))
    assert es <= 4.0 * max(ns, 2.0 ** -54) and ec <= 4.0 * max(nc, 2.0 ** -54)
    assert s[0] == 0.0 and c[0] == 1.0
    # near the cutoff the force is made of pi - arg: right relative to the small value
    near = np.pi - np.array([1e-3, 1e-6, 1e-9, 1e-12])
    s2, c2 = np.zeros_like(near), np.zeros_like(near)
    lib.lammps_le_test_soft_sincos(len(near), near.ctypes.data_as(PD), s2.ctypes.data_as(PD), c2.ctypes.data_as(PD))
    assert (np.abs(s2 / np.sin(near.astype(LD)).astype(np.float64) - 1.0) < 4e-16).all()


# ------------------------------------------------------------------------------------------------------------------
# 3. the step plan
# ------------------------------------------------------------------------------------------------------------------
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_STEP_LDS_PAD", "LAMMPS_LE_DIAG_STEP")


def _hooks():
    lib = _lib()
    out = []
    for name, nreq, nout in (("lammps_le_test_step_plan", 11, 16), ("lammps_le_test_step_plan_walls", 12, 18), ("lammps_le_test_step_plan_soft", 13, 19)):
        fn = getattr(lib, name)
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        fn.restype = None

        def plan(n, dd, r, fn=fn, nreq=nreq, nout=nout):
            req, res = (ctypes.c_int * nreq)(*r), (ctypes.c_int * nout)()
            fn(n, dd, req, res)
            return list(res)
        out.append(plan)
    return out


@pytest.mark.parametrize("env", [{}, {"LAMMPS_LE_LPB": "1"}, {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}, {"LAMMPS_LE_NO_FUSE": "1"},
                                 {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0", "LAMMPS_LE_DIAG_STEP": "8"}])
def test_step_plan_with_soft(monkeypatch, env):
    """Every request: without soft the new hook answers as the two old ones; a soft request is fused exactly where it is a plain
    step with a pair style - no thermo, angles, groups, walls -, the fused plan names an instantiation the dispatcher holds, is
    the lj/cut plan in everything but the soft flag, never claims pending velocities and never comes with the diagnostic launch;
    over all requests the fused answers are the 24 shapes L, N, I x {four lanes, one lane ahead, one lane}."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    old, walls, soft = _hooks()
    shapes = set()
    for n, dd in itertools.product((1000, 50001, 1000000), (0, 1)):
        for L, N, I, P, angles, thermo, check, cells in itertools.product((0, 1), repeat=8):
            for nvebit, lgbit, which in ((1, 1, -1), (2, 1, -1), (1, 2, -1), (1, 1, 1)):
                r = [L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells]
                base = old(n, dd, r)
                for w in (0, 1, 2):
                    assert soft(n, dd, r + [w, 0])[:18] == walls(n, dd, r + [w]) and soft(n, dd, r + [w, 0])[18] == 0
                assert soft(n, dd, r + [1, 1])[0] == 0 and soft(n, dd, r + [2, 1])[0] == 0          # walls together with soft
                s = soft(n, dd, r + [0, 1])
                if thermo or angles or not P or nvebit != 1 or lgbit != 1 or "LAMMPS_LE_NO_FUSE" in env:
                    assert s[0] == 0, (r, s)
                    continue
                assert s[0] == 1 and s[18] == 1 and s[15] == 1, (r, s)          # fused, soft, the instantiation exists
                assert s[1:13] == base[1:13] and s[14] == base[14], (r, s, base)
                assert s[13] == 0 and s[16] == 0 and s[17] == 0, (r, s)          # no diagnostic launch, no wall, no velocity hand-over
                assert s[8] == s[9] == s[10] == s[6] == 0
                shapes.add((s[1], s[2], s[3], s[5], s[7]))
    if "LAMMPS_LE_NO_FUSE" in env:
        assert not shapes
    else:
        assert all(lpb == 1 or ahead for _, _, _, lpb, ahead in shapes)
        if not env:
            assert len(shapes) == 24, sorted(shapes)


# ------------------------------------------------------------------------------------------------------------------
# 4. the script layer
# ------------------------------------------------------------------------------------------------------------------
def _open(tmp_path, n=125, types=None, script=CHAIN_SCRIPT):
    from lammps_le_amd import lammps
    path = os.path.join(str(tmp_path), "data.chain")
    write_data(path, lattice_chain(n, types=types))
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in script.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp


def _coeffs(lmp, phase=0, begin=0, end=0, now=0):
    """(6, nt, nt): the derived pair table the script layer holds (lammps_le_test_pair_coeffs)"""
    fn = lmp.lib.lammps_le_test_pair_coeffs
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_long, PD]
    fn.restype = ctypes.c_int
    out = np.zeros(6 * 64)
    nt = fn(lmp.lmp, phase, begin, end, now, out.ctypes.data_as(PD))
    lmp._check()
    assert nt > 0
    return out[:6 * nt * nt].reshape(6, nt, nt)


def _refused(lmp, line, text):
    from lammps_le_amd import LammpsError
    with pytest.raises(LammpsError, match=text):
        lmp.command(line)


THREE = np.array(([1, 2, 3] * 42)[:125])


def test_soft_coefficients_and_mixing(tmp_path):
    """pair_coeff I J A [rc] with wildcards; unset pairs: A geometric under both mix settings, rc by pair_modify mix; no offset
    under shift yes; the table columns cutsq, A pi/rc, pi/rc, A; the reference's errors."""
    lmp = _open(tmp_path, types=THREE)
    assert lmp.has_style("pair", "soft") and lmp.has_style("fix", "adapt")
    _refused(lmp, "pair_style soft", "Illegal pair_style command")
    _refused(lmp, "pair_style soft 1.0 2.0", "Illegal pair_style command")
    lmp.command("pair_style soft 1.12246")
    _refused(lmp, "pair_coeff 1 1", "Incorrect args for pair coefficients")
    _refused(lmp, "pair_coeff 1 1 1.0 1.0 1.0", "Incorrect args for pair coefficients")
    _refused(lmp, "pair_coeff 2 1 1.0", "Incorrect args for pair coefficients")          # (no pair with i <= j)
    _refused(lmp, "pair_coeff 1 4 1.0", "Numeric index is out of bounds")
    lmp.command("pair_coeff 1 1 4.0 1.0")
    lmp.command("pair_coeff 2 2 9.0 1.44")
    _refused(lmp, "run 0", "All pair coeffs are not set")
    lmp.command("pair_coeff 3 3 16.0")
    lmp.command("pair_coeff 1 3 5.0 1.3")
    lmp.command("pair_modify shift yes")
    for mix, rc12 in (("geometric", np.sqrt(1.0 * 1.44)), ("arithmetic", 0.5 * (1.0 + 1.44))):
        lmp.command("pair_modify mix " + mix)
        t = _coeffs(lmp)
        a = {(1, 1): 4.0, (2, 2): 9.0, (3, 3): 16.0, (1, 3): 5.0, (1, 2): 6.0, (2, 3): 12.0}
        rc23 = np.sqrt(1.44 * 1.12246) if mix == "geometric" else 0.5 * (1.44 + 1.12246)
        rc = {(1, 1): 1.0, (2, 2): 1.44, (3, 3): 1.12246, (1, 3): 1.3, (1, 2): rc12, (2, 3): rc23}
        for (i, j), av in a.items():
            for p, q in ((i, j), (j, i)):
                assert t[0, p, q] == rc[(i, j)] * rc[(i, j)] and t[3, p, q] == av
                assert t[1, p, q] == av * np.pi / rc[(i, j)] and t[2, p, q] == np.pi / rc[(i, j)]
                assert t[4, p, q] == 0.0 and t[5, p, q] == 0.0          # no offset: pair_modify shift has nothing to shift
    # wildcards set every pair, a later row overrides
    lmp.command("pair_style soft 2.5")
    lmp.command("pair_coeff * * 7.0")
    lmp.command("pair_coeff 2*3 3 1.0 0.5")
    t = _coeffs(lmp)
    assert (t[3, 1:, 1:] == np.array([[7, 7, 7], [7, 7, 1], [7, 1, 1]])).all() and t[0, 1, 1] == 6.25 and t[0, 3, 2] == 0.25
    # rows of interacting pairs are lj/cut's
    lmp.command("compute pl all pair/local dist eng")
    _refused(lmp, "run 0", "MI355X engine: compute pair/local rows of interacting pairs are not supported under pair_style soft")
    lmp.command("uncompute pl")
    lmp.command("compute pp all property/local patom1 patom2")
    _refused(lmp, "run 0", "MI355X engine: compute property/local rows of interacting pairs are not supported under pair_style soft")
    lmp.close()


def test_style_switch_on_one_handle(tmp_path):
    """soft -> lj/cut -> soft: each style starts with no coefficients and derives its own table"""
    lmp = _open(tmp_path)
    lj = _coeffs(lmp)
    assert lj[1, 1, 1] == 48.0 and lj[5, 1, 1] != 0.0
    lmp.command("pair_style soft 1.12246")
    _refused(lmp, "run 0", "All pair coeffs are not set")
    lmp.command("pair_coeff * * 3.0")
    s = _coeffs(lmp)
    assert s[3, 1, 1] == 3.0 and s[4, 1, 1] == 0.0 and s[5, 1, 1] == 0.0 and s[0, 1, 1] == 1.12246 ** 2
    lmp.command("pair_style lj/cut 1.12")
    _refused(lmp, "run 0", "All pair coeffs are not set")
    lmp.command("pair_coeff * * 1.0 1.0 1.12")
    assert np.array_equal(_coeffs(lmp), lj)
    lmp.command("pair_style soft 1.12246")
    lmp.command("pair_coeff * * 3.0")
    assert np.array_equal(_coeffs(lmp), s)
    lmp.close()


def test_ramp_between_runs_and_in_a_run(tmp_path):
    lmp = _open(tmp_path)
    lmp.command("variable A equal ramp(0,60)")
    _refused(lmp, "print $A", "Cannot use ramp in variable formula between runs")
    lmp.command("variable B equal ramp(1)")
    _refused(lmp, "print $B", "Invalid math function in variable formula")
    lmp.command("pair_style soft 1.12246")
    lmp.command("pair_coeff * * 0.0")
    lmp.command("fix push all adapt 1 pair soft a * * v_A")
    _coeffs(lmp)
    # x + (y - x) (step - beginstep) / (endstep - beginstep): a run over steps 100 .. 300
    assert _coeffs(lmp, 1, 100, 300)[3, 1, 1] == 0.0
    assert _coeffs(lmp, 2, 100, 300, 150)[3, 1, 1] == 0.0 + (150 - 100) / (300 - 100) * 60.0
    assert _coeffs(lmp, 2, 100, 300, 300)[3, 1, 1] == 60.0
    _refused(lmp, "print $A", "Cannot use ramp in variable formula between runs")
    lmp.close()


def test_fix_adapt_grammar_and_refusals(tmp_path):
    lmp = _open(tmp_path, types=THREE)
    lmp.command("pair_style soft 1.12246")
    lmp.command("pair_coeff * * 1.0")
    lmp.command("variable A equal ramp(0,60)")
    lmp.command("variable T equal 2.0*temp")
    lmp.command("variable P equal v_A+press")
    lmp.command("variable name index hello")
    lmp.command("fix 1 all nve")
    ill = "Illegal fix adapt command"
    _refused(lmp, "fix a all adapt", ill)
    _refused(lmp, "fix a all adapt -1 pair soft a * * v_A", ill)
    _refused(lmp, "fix a all adapt 1 pair soft a * *", ill)
    _refused(lmp, "fix a all adapt 1 pair soft a * * A", ill)                     # (not v_name)
    _refused(lmp, "fix a all adapt 1 reset yes", ill)
    _refused(lmp, "fix a all adapt 1 pair soft a * * v_A reset maybe", ill)
    _refused(lmp, "fix a all adapt 1 pair soft a * * v_A frobnicate yes", ill)
    _refused(lmp, "fix a all adapt 1 pair soft a 1 4 v_A", "Numeric index is out of bounds")
    _refused(lmp, "fix a nobody adapt 1 pair soft a * * v_A", "Could not find fix group ID")
    _refused(lmp, "fix a all adapt 1 bond fene k * v_A", "MI355X engine: fix adapt bond is not supported")
    _refused(lmp, "fix a all adapt 1 kspace v_A", "MI355X engine: fix adapt kspace is not supported")
    _refused(lmp, "fix a all adapt 1 atom diameter v_A", "MI355X engine: fix adapt atom is not supported")
    _refused(lmp, "fix a all adapt 1 pair lj/cut/coul/long epsilon * * v_A", "MI355X engine: fix adapt pair style lj/cut/coul/long is not supported")
    _refused(lmp, "fix a all adapt 1 pair soft epsilon * * v_A", "MI355X engine: Fix adapt pair style param not supported")
    _refused(lmp, "fix a all adapt 1 pair lj/cut a * * v_A", "MI355X engine: Fix adapt pair style param not supported")
    # said at the run: the variable, its style, the pair style in force, a formula that reads the device
    for line, text in (("fix a all adapt 1 pair soft a * * v_nosuch", "Variable name for fix adapt does not exist"),
                       ("fix a all adapt 1 pair soft a * * v_name", "Variable for fix adapt is invalid style"),
                       ("fix a all adapt 1 pair lj/cut epsilon * * v_A", "Fix adapt pair style does not exist"),
                       ("fix a all adapt 1 pair soft a * * v_T", "MI355X engine: variable T of fix adapt reads temp"),
                       ("fix a all adapt 1 pair soft a * * v_P", "MI355X engine: variable P of fix adapt reads press")):
        lmp.command(line)
        _refused(lmp, "run 10", text)
        lmp.command("unfix a")
    lmp.command("fix w all langevin 1.0 1.0 1.0 12345")
    lmp.command("variable F equal f_w")
    lmp.command("fix a all adapt 1 pair soft a * * v_F")
    _refused(lmp, "run 10", "MI355X engine: variable F of fix adapt reads f_w")
    lmp.command("unfix a")
    # what the host can evaluate: step, elapsed, dt, time, the math functions, other such variables
    lmp.command("variable H equal 0.5*v_A+sqrt(step)+elapsed*dt+time+min(1,2)")
    lmp.command("fix a all adapt 3 pair soft a * * v_H")
    _coeffs(lmp)
    got = _coeffs(lmp, 2, 0, 100, 9)[3, 1, 1]
    assert got == 0.5 * (9 / 100 * 60.0) + 3.0 + 9 * 0.005 + 9 * 0.005 + 1
    lmp.close()


def test_fix_adapt_values(tmp_path):
    """scale, reset, N = 0, two pair clauses; after every change all type pairs are derived again, mixing included."""
    lmp = _open(tmp_path, types=THREE)
    lmp.command("pair_style soft 1.12246")
    lmp.command("pair_coeff 1 1 4.0")
    lmp.command("pair_coeff 2 2 9.0 1.3")
    lmp.command("pair_coeff 3 3 1.0")
    lmp.command("pair_coeff 1 3 2.0")
    lmp.command("variable A equal ramp(1,3)")
    lmp.command("variable B equal ramp(10,20)")
    # two clauses, scale yes: the values FixAdapt::init finds are multiplied
    lmp.command("fix a all adapt 2 pair soft a 1 1 v_A pair soft a 2*3 3 v_B scale yes reset yes")
    base = _coeffs(lmp)
    assert base[3, 1, 2] == 6.0 and base[3, 2, 3] == 3.0
    t = _coeffs(lmp, 1, 0, 10)                                   # setup: ramp at its start
    assert t[3, 1, 1] == 4.0 and t[3, 3, 3] == 10.0 and t[3, 2, 2] == 9.0 and t[3, 1, 3] == 2.0
    assert t[3, 2, 3] == np.sqrt(9.0 * 10.0)                     # 2-3 is unset: what the clause writes there is replaced by mixing,
    t = _coeffs(lmp, 2, 0, 10, 4)                                # sqrt(A22 A33) of the moment
    va, vb = 1.0 + 4 / 10 * (3.0 - 1.0), 10.0 + 4 / 10 * (20.0 - 10.0)
    assert t[3, 1, 1] == va * 4.0 and t[3, 3, 3] == vb * 1.0
    assert t[3, 2, 3] == np.sqrt(9.0 * vb) and t[3, 1, 2] == np.sqrt(va * 4.0 * 9.0) and t[3, 2, 1] == t[3, 1, 2]
    assert t[1, 1, 1] == va * 4.0 * np.pi / 1.12246 and t[0, 2, 2] == 1.3 * 1.3          # rc is not adapted
    # N = 2: step 7 is not its step - the hook's phase 2 at a step that is not due leaves the table alone
    assert np.array_equal(_coeffs(lmp, 2, 0, 10, 7), t)
    # reset yes: post_run restores what init found
    assert np.array_equal(_coeffs(lmp, 3, 0, 10, 10), base)
    lmp.command("unfix a")
    # N = 0: at setup only; scale no: the value itself
    lmp.command("fix a all adapt 0 pair soft a * * v_B")
    _coeffs(lmp)
    t0 = _coeffs(lmp, 1, 0, 10)
    assert (t0[3, 1:, 1:] == 10.0).all()
    assert np.array_equal(_coeffs(lmp, 2, 0, 10, 5), t0)
    # reset no: the values stay, and the next run's init takes them for the original ones (FixAdapt::init copies what it finds)
    assert np.array_equal(_coeffs(lmp, 3, 0, 10, 10), t0)
    lmp.close()


def test_fix_adapt_lj_cut(tmp_path):
    """lj/cut epsilon and sigma: lj1 .. lj4 and the shift offset follow; the cutoff and with it the list do not"""
    lmp = _open(tmp_path, types=THREE)
    lmp.command("pair_style lj/cut 2.5")
    lmp.command("pair_modify shift yes")
    lmp.command("pair_coeff * * 1.0 1.0")
    lmp.command("pair_coeff 1 2 0.5 1.0 1.5")
    lmp.command("variable E equal ramp(0,2)")
    lmp.command("variable S equal 0.9")
    lmp.command("fix a all adapt 1 pair lj/cut epsilon 1 2 v_E pair lj/cut sigma 3 3 v_S")
    _coeffs(lmp)
    t = _coeffs(lmp, 2, 0, 4, 3)
    eps, sig = 1.5, 0.9
    assert t[1, 1, 2] == 48.0 * eps and t[2, 2, 1] == 24.0 * eps and t[0, 1, 2] == 2.25
    assert t[5, 1, 2] == 4.0 * eps * ((1.0 / 1.5) ** 12.0 - (1.0 / 1.5) ** 6.0)
    assert t[1, 3, 3] == 48.0 * sig ** 12.0 and t[0, 3, 3] == 6.25
    assert t[1, 1, 1] == 48.0 and t[1, 2, 3] == 48.0          # set pairs keep their own values
    lmp.close()


def test_restart_round_trip(tmp_path):
    """The style name and the current coefficients travel, as lj/cut's do; fix adapt is given again after read_restart."""
    from lammps_le_amd import lammps
    lmp = _open(tmp_path, types=THREE)
    lmp.command("pair_style soft 1.12246")
    lmp.command("pair_modify mix arithmetic")
    lmp.command("pair_coeff 1 1 4.0")
    lmp.command("pair_coeff 2 2 9.0 1.3")
    lmp.command("pair_coeff 3 3 1.0")
    lmp.command("variable A equal ramp(1,3)")
    lmp.command("fix a all adapt 1 pair soft a 1 1 v_A")
    _coeffs(lmp)
    want = _coeffs(lmp, 2, 0, 10, 5)          # the coefficients of the moment: A11 = 2
    path = os.path.join(str(tmp_path), "soft.restart")
    lmp.command("write_restart " + path)
    lmp.close()
    lmp = lammps(cmdargs=["-screen", "none"])
    lmp.command("read_restart " + path)
    assert lmp.available_ids("fix") == []
    got = _coeffs(lmp)
    assert np.array_equal(got, want) and got[3, 1, 1] == 2.0 and got[0, 1, 2] == (0.5 * (1.12246 + 1.3)) ** 2
    lmp.command("pair_style lj/cut 1.12")
    lmp.command("pair_coeff * * 1.0 1.0")
    path2 = os.path.join(str(tmp_path), "lj.restart")
    lmp.command("write_restart " + path2)
    lmp.close()
    lmp = lammps(cmdargs=["-screen", "none"])
    lmp.command("read_restart " + path2)
    assert _coeffs(lmp)[1, 1, 1] == 48.0 and _coeffs(lmp)[4, 1, 1] == 4.0
    lmp.close()


def test_parent_restart_file_still_reads():
    """tests/golden/parent_lj.restart was written by the commit before pair_style soft existed (125 beads, lj/cut 1.12 shifted,
    FENE): it reads, as lj/cut, with its coefficients."""
    from lammps_le_amd import lammps
    lmp = lammps(cmdargs=["-screen", "none"])
    lmp.command("read_restart " + os.path.join(G, "parent_lj.restart"))
    assert lmp.get_natoms() == 125
    t = _coeffs(lmp)
    assert t[1, 1, 1] == 48.0 and t[0, 1, 1] == 1.12 * 1.12 and t[5, 1, 1] != 0.0
    lmp.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the fixtures
# ------------------------------------------------------------------------------------------------------------------
def test_conditions_on_the_run0_fixture():
    """At least 15 pairs below half their cutoff, the coincident pair, an interacting pair at each special level; the figure
    soft_runs.json holds for the recorded reference run against the long-double reference is there and small."""
    s, moved, same = so.soft_system(True)
    S, ev, _ = so.a_reference()
    assert so.a_conditions(S, ev, s, moved, same) == ""
    fx, m = so.fixture("a"), so.meta()["a"]
    # the fixture states them, and they are those of the input as it is built here
    c = m["conditions"]
    assert c == so.a_counts(S, ev, s, same)
    assert c["below_half_cutoff"] >= 15 and c["coincident"] == 1
    assert min(c["level_1_3"], c["level_1_4"], c["unweighted"], c["bonded_within_cutoff"]) >= 1
    assert fx["f"].shape == (so.wl.A_N, 3) and np.isfinite(fx["f"]).all()
    assert 0 < m["reference_deviation"]["f"] < 1e-13 and m["beads"] == so.wl.A_N
    # the long-double reference and the recorded run agree to that figure (it is where the GPU bounds come from)
    assert fc.relerr(fx["f"], ev.f) <= m["reference_deviation"]["f"]


@pytest.mark.parametrize("name", so.NAMES)
def test_conditions_on_the_recorded_runs(name):
    fx, scn = so.fixture(name), so.BY_NAME[name]
    assert so.b_conditions(fx, scn) == ""
    m = so.meta()["scenarios"][name]
    assert m["steps"] == so.last_step(scn) and m["perturbed_reruns"] == 3
    assert np.array_equal(fx["start_x"], so.b_system()["x"])


@pytest.mark.parametrize("n,nchains", [(2000, 1), (3000, 3)])
def test_phantom_chains(n, nchains):
    """What synth.phantom_chains promises: bond length 0.97, bead i farther than 1.02 from bead i - 2 (within a chain), bonds
    inside chains only, coordinates wrapped into the box with image flags that undo the wrap, a box of volume n / density
    centred on the origin, overlapping beads (it is NOT a start lj/cut survives), the same walk for the same seed."""
    from lammps_le_amd.synth import phantom_chains
    s = phantom_chains(n, nchains, 0.85, seed=7)
    box = np.asarray(s["box"], dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    assert np.allclose(prd, (n / 0.85) ** (1.0 / 3.0)) and np.allclose(box[:, 0], -box[:, 1])
    x = np.asarray(s["x"])
    assert x.shape == (n, 3) and (x >= box[:, 0]).all() and (x < box[:, 1]).all()
    xu = x + np.asarray(s["image"]) * prd
    per = n // nchains
    bonds = np.asarray(s["bonds"])
    assert len(bonds) == n - nchains and (bonds[:, 2] == bonds[:, 1] + 1).all() and (bonds[:, 0] == 1).all()
    assert ((bonds[:, 1] - 1) // per == (bonds[:, 2] - 1) // per).all()          # no bond across a chain end
    blen = np.sqrt(((xu[bonds[:, 2] - 1] - xu[bonds[:, 1] - 1]) ** 2).sum(axis=1))
    assert np.abs(blen - 0.97).max() < 1e-12
    i = np.arange(n - 2)
    same_chain = i // per == (i + 2) // per
    d2 = np.sqrt(((xu[i + 2] - xu[i]) ** 2).sum(axis=1))[same_chain]
    assert d2.min() > 1.02 and d2.max() <= 2 * 0.97 + 1e-12
    assert np.asarray(s["image"]).any() and len(s["v"]) == n and abs(np.asarray(s["v"]).mean()) < 1e-12
    assert so.closest_nonbonded(x, s["box"], s["bonds"]) < 0.2
    again = phantom_chains(n, nchains, 0.85, seed=7)
    assert np.array_equal(again["x"], x) and not np.array_equal(phantom_chains(n, nchains, 0.85, seed=8)["x"], x)
    with pytest.raises(ValueError):
        phantom_chains(n + 1, nchains if nchains > 1 else 2, 0.85)


def test_conditions_on_the_push_off_record():
    m = so.meta()["push"]
    assert m["closest_after_stage1"] >= so.PUSH_CLOSEST_REFERENCE and m["steps"] >= 1000 and m["fene_warnings_stage2"] == 0
    s = so.push_system()
    assert so.closest_nonbonded(s["x"], s["box"], s["bonds"]) < 0.1          # the start does overlap
