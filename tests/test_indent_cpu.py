"""fix indent without a device: the script layer's grammar and error strings through the C-ABI, vdisplace() in formulas, the
step plan with indenters against the instantiations of the step kernel (test hook lammps_le_test_step_plan_indent; nothing is
launched), indent_force of indent_inl.h compiled for the host against long double (lammps_le_test_indent_force), the long-double
restatement (indent_reference.py) against the recorded `run 0` of the reference binary, the conditions the fixtures were made
under (indent_runs.py) and - where the reference binary has been built - the regeneration of one fixture of each kind."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

import indent_reference as ir
import indent_runs as ind
from systems import CHAIN_SCRIPT, lattice_chain, write_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")
# the project's bound for single evaluations against reference-held vectors, relative to max(1, |value|)
RUN0_BOUND = 1e-12


def _open(tmp_path, n=125):
    from lammps_le_amd import lammps
    path = os.path.join(str(tmp_path), "data.chain")
    write_data(path, lattice_chain(n))
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in CHAIN_SCRIPT.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp


def _refuser(lmp):
    from lammps_le_amd import LammpsError

    def refused(line, text):
        with pytest.raises(LammpsError, match=text):
            lmp.command(line)
    return refused


def test_grammar_and_error_strings(tmp_path):
    lmp = _open(tmp_path)
    refused = _refuser(lmp)
    assert lmp.has_style("fix", "indent")
    lmp.command("fix 1 all nve")
    ill = "Illegal fix indent command"
    # src/fix_indent.cpp:45, :84, options :405-528
    refused("fix c all indent", ill)
    refused("fix c all indent 10.0", ill)                              # (no shape)
    refused("fix c all indent 10.0 side in", ill)
    refused("fix c all indent 10.0 sphere 1 2 3", ill)
    refused("fix c all indent 10.0 cylinder w 1 2 3", ill)
    refused("fix c all indent 10.0 cylinder z 1 2", ill)
    refused("fix c all indent 10.0 plane x 1.0", ill)
    refused("fix c all indent 10.0 plane x 1.0 mid", ill)
    refused("fix c all indent 10.0 plane w 1.0 lo", ill)
    refused("fix c all indent 10.0 sphere 1 2 3 4 side", ill)
    refused("fix c all indent 10.0 sphere 1 2 3 4 side up", ill)
    refused("fix c all indent 10.0 sphere 1 2 3 4 units", ill)
    refused("fix c all indent 10.0 sphere 1 2 3 4 units reduced", ill)
    refused("fix c all indent 10.0 sphere 1 2 3 4 cone", ill)
    refused("fix c nobody indent 10.0 sphere 1 2 3 4", "Could not find fix group ID")
    # the keywords in any order, both units
    for k, line in enumerate(("side in units box sphere 3 3 3 9", "cylinder y 3 3 1.0 units lattice", "plane z 0.5 lo side out", "units box plane x 5 hi")):
        lmp.command("fix c%d all indent 10.0 %s" % (k, line))
    refused("fix c4 all indent 1.0 sphere 3 3 3 1", "at most 4 fix indent")            # INDENT_MAX
    assert lmp.available_ids("fix") == ["1", "c0", "c1", "c2", "c3"]
    # fix_modify (src/fix.cpp:134-176): THERMO_ENERGY, no virial_flag; respa in the engine's words
    lmp.command("fix_modify c0 energy yes")
    lmp.command("fix_modify c0 energy no virial no")
    refused("fix_modify c0 virial yes", "Illegal fix_modify command")
    refused("fix_modify c0 energy maybe", "Illegal fix_modify command")
    refused("fix_modify c0 respa 1", "MI355X engine: fix_modify respa is not supported")
    # f_ID and f_ID[1..3]; beyond that the reference's words
    lmp.command("thermo_style custom step pe f_c0 f_c0[1] f_c0[3]")
    lmp.command("variable e equal f_c0+f_c0[2]")
    assert lmp.extract_fix("c0", 0, 0) == 0.0 and lmp.extract_fix("c0", 0, 1, 2) == 0.0
    lmp.command("variable bad equal f_c0[4]")
    refused("print ${bad}", "Variable formula fix vector is accessed out-of-range")
    from lammps_le_amd import LammpsError
    with pytest.raises(LammpsError, match="out-of-range"):
        lmp.extract_fix("c0", 0, 1, 3)
    lmp.close()


def test_variables_are_checked_at_run(tmp_path):
    """FixIndent::init's three texts, and the engine's refusal of a formula that reads the device - fix adapt's message word for
    word, with the style's name in it."""
    lmp = _open(tmp_path)
    refused = _refuser(lmp)
    lmp.command("fix 1 all nve")
    lmp.command("variable R equal ramp(9,7)")
    lmp.command("variable S index 4.0")
    lmp.command("variable T equal 0.5*temp")
    lmp.command("variable F equal f_1[1]")

    def with_fix(line, text):
        lmp.command("fix c all indent 10.0 " + line)
        refused("run 0", text)
        refused("minimize 0 0 1 1", text)
        lmp.command("unfix c")
    with_fix("sphere 3 3 3 v_none", "Variable name for fix indent does not exist")
    with_fix("sphere v_none 3 3 2", "Variable name for fix indent does not exist")
    with_fix("sphere v_S 3 3 2", "Variable for fix indent is invalid style")
    with_fix("sphere 3 v_S 3 2", "Variable for fix indent is not equal style")
    with_fix("sphere 3 3 v_S 2", "Variable for fix indent is not equal style")
    with_fix("cylinder z 3 3 v_S", "Variable for fix indent is not equal style")
    with_fix("plane x v_S lo", "Variable for fix indent is not equal style")
    with_fix("sphere 3 3 3 v_T", r"MI355X engine: variable T of fix indent reads temp, which lives on the device \(numbers, step, elapsed, "
                                 r"dt, time, ramp\(\) and the math functions are evaluated per step\)")
    with_fix("plane y v_F hi", "MI355X engine: variable F of fix indent reads f_1, which lives on the device")
    # fix adapt's message stays what it was
    lmp.command("pair_style soft 1.12")
    lmp.command("pair_coeff * * 1.0")
    lmp.command("fix a all adapt 1 pair soft a * * v_T")
    refused("run 0", r"MI355X engine: variable T of fix adapt reads temp, which lives on the device \(numbers, step, elapsed, dt, time, "
                     r"ramp\(\) and the math functions are evaluated per step\)")
    lmp.close()


def test_order_against_addforce_and_setforce(tmp_path):
    """Within one side of fix langevin an indenter must be defined ahead of an addforce or setforce, like a wall."""
    lmp = _open(tmp_path)
    refused = _refuser(lmp)
    for line in ("fix 1 all nve", "fix a all addforce 0 0 1", "fix c all indent 10.0 sphere 3 3 3 9 side in"):
        lmp.command(line)
    refused("run 0", r"MI355X engine: fix c \(indent\) is defined behind a fix addforce or setforce on the same side of fix langevin")
    lmp.close()


def test_vdisplace(tmp_path):
    """vdisplace(x, v) = x + v * (step - beginstep) * dt (src/variable.cpp:3743-3754): between runs the reference's refusal;
    swiggle / cwiggle stay unknown functions."""
    lmp = _open(tmp_path)
    refused = _refuser(lmp)
    lmp.command("variable d equal vdisplace(2.0,3.0)")
    lmp.command("variable w equal swiggle(0.0,1.0,2.0)")
    lmp.command("variable one equal vdisplace(2.0)")
    refused("print ${d}", "Cannot use vdisplace in variable formula between runs")
    refused("print ${one}", "Invalid math function in variable formula")
    refused("print ${w}", "Invalid math function in variable formula")
    lmp.command("variable m equal min(1,2,3)")          # (a third argument to a function the parser has: the syntax error it always was)
    refused("print ${m}", "Invalid syntax in variable formula")
    # inside a run: the table the force evaluation of a step would carry (test hook, no device) - an obstacle whose centre
    # moves by vdisplace, written one period below the box so that Domain::remap acts, and a plane on a ramp
    L = float(lattice_chain(125)["box"][0][1])
    lmp.command("fix 1 all nve")
    lmp.command("variable X equal vdisplace(%.17g,3.0)" % (2.0 - L))
    lmp.command("variable P equal ramp(4.0,2.0)")
    lmp.command("fix 2 all langevin 1.0 1.0 1.0 4242")
    lmp.command("fix ob all indent 1.5 sphere v_X 1.0 %.17g 0.75 side out" % (L + 0.5))
    lmp.command("group some id 1:125:2")
    lmp.command("fix pl some indent 6.0 plane y v_P hi")
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_indent_table
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.POINTER(ctypes.c_double)]
    out = (ctypes.c_double * 40)()
    for now in (100, 140, 200):
        assert fn(lmp.lmp, 100, 200, now, out) == 2
        a, b = list(out[:10]), list(out[10:20])
        x = (2.0 - L) + 3.0 * float(now - 100) * 0.005
        assert a[:6] == [0, 0, 0, 1, 1, 1.5] and a[6:] == [x + L, 1.0, (L + 0.5) - L, 0.75], (now, a)
        delta = float(now - 100) / 100.0 if now != 100 else 0.0
        assert b[:6] == [2, 1, 1, 2, 1, 6.0] and b[9] == 4.0 + delta * (2.0 - 4.0), (now, b)
    # a ramp cut in the middle and given again with its remaining span starts where the first half ended (what a restart in the
    # middle of a compaction relies on): ramp(4, 2) at step 150 of [100, 200] is ramp(3, 2) at step 150 of [150, 200]
    assert fn(lmp.lmp, 100, 200, 150, out) == 2
    half = out[19]
    lmp.command("variable P delete")
    lmp.command("variable P equal ramp(%.17g,2.0)" % half)
    assert fn(lmp.lmp, 150, 200, 150, out) == 2 and out[19] == half == 3.0
    lmp.close()


# ------------------------------------------------------------------------------------------------------------------
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_STEP_LDS_PAD", "LAMMPS_LE_DIAG_STEP")


def _hook(name, nreq, nout):
    from lammps_le_amd import library_path
    fn = getattr(ctypes.CDLL(library_path()), name)
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = None

    def plan(n, dd, r):
        req, res = (ctypes.c_int * nreq)(*r), (ctypes.c_int * nout)()
        fn(n, dd, req, res)
        return list(res)
    return plan


@pytest.mark.parametrize("env", [{}, {"LAMMPS_LE_LPB": "1"}, {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}, {"LAMMPS_LE_NO_FUSE": "1"}])
def test_step_plan_with_indenters(monkeypatch, env):
    """Fix indent has a bit of the kernel's key of its own, so that a wall variant without indenters stays the code it was.  indents = 1
    gives, request by request, the plan walls = 1 gives (so it fuses in exactly the shapes walls = 1 does) with StepPlan::indent
    set on top, alone and together with walls = 1, and the dispatcher holds the instantiation; indents = 2, and indents = 1
    beside walls = 2, never fuse; thermo steps, angle styles, pair_style soft and the force fixes do not fuse with an indenter;
    without indenters the hook answers as the one before it and no plan has the flag.  The instantiations without that
    bit are still 153; with the 24 indent variants (L, N, I x three shapes) there are 177."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    old, new = _hook("lammps_le_test_step_plan_ext", 14, 21), _hook("lammps_le_test_step_plan_indent", 15, 23)
    fused = 0
    for n, dd in itertools.product((1000, 50001, 1000000), (0, 1)):
        for L, N, I, P, angles, thermo, check, cells in itertools.product((0, 1), repeat=8):
            for nvebit, lgbit, which in ((1, 1, -1), (2, 1, -1), (1, 1, 1)):
                r = [L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells]
                for walls, soft, ext in itertools.product((0, 1, 2), (0, 1), (0, 1)):
                    got = new(n, dd, r + [walls, soft, ext, 0])
                    assert got[:21] == old(n, dd, r + [walls, soft, ext]) and got[21] == 0 and got[22] == 177
                wall_plan = old(n, dd, r + [1, 0, 0])
                assert wall_plan[20] == 153
                for walls in (0, 1):
                    got = new(n, dd, r + [walls, 0, 0, 1])
                    assert got[:21] == wall_plan and got[21] == wall_plan[0], (r, walls, got)      # (got[15]: the instantiation exists)
                    assert new(n, dd, r + [walls, 0, 0, 2])[0] == 0
                    assert new(n, dd, r + [walls, 1, 0, 1])[0] == 0 and new(n, dd, r + [walls, 0, 1, 1])[0] == 0
                assert new(n, dd, r + [2, 0, 0, 1])[0] == 0
                if thermo or angles:
                    assert wall_plan[0] == 0
                if wall_plan[0]:
                    assert wall_plan[15] == 1 and wall_plan[16] == 1
                fused += wall_plan[0] and wall_plan[16]
    assert fused > 0 or "LAMMPS_LE_NO_FUSE" in env


# ------------------------------------------------------------------------------------------------------------------
def _host_indent_force(x, o, box):
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_indent_force
    PD = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [ctypes.c_int, PD, PD, PD, PD, PD, PD]
    fn.restype = None
    x = np.ascontiguousarray(x, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    lo, hi = np.ascontiguousarray(box[:, 0]), np.ascontiguousarray(box[:, 1])
    kind = ("sphere", "cylinder", "plane").index(o["kind"])
    side = o["planeside"] if kind == 2 else int(o["side"] == "in")
    ctr = o.get("ctr", [0.0, 0.0, 0.0])
    geo = np.array([kind, o.get("dim", 0), side, o["K"], ctr[0], ctr[1], ctr[2], o["pos"] if kind == 2 else o["R"]], dtype=np.float64)
    f, sums = np.zeros_like(x), np.zeros(4)
    fn(len(x), x.ctypes.data_as(PD), lo.ctypes.data_as(PD), hi.ctypes.data_as(PD), geo.ctypes.data_as(PD), f.ctypes.data_as(PD), sums.ctypes.data_as(PD))
    return f, sums


@pytest.mark.parametrize("case", list(ind.A_CASES))
def test_indent_force_on_the_host(case):
    """indent_force of indent_inl.h - the function the kernels run, compiled for the host without contraction - against the
    long-double restatement on the (a) system with every bead a member, and on 4000 random points of the box and its surroundings
    (up to one period outside, where the minimum image takes more than one trip).  A force component is a product of four
    factors and a quotient, each rounded once, the sums add at most 4000 such terms: 1e-12 relative to max(1, |value|), the
    project's bound for a single evaluation.  Measured: at most 2.3e-15 (forces), 1.3e-14 (sums)."""
    s = ind.a_system()
    o = ind.a_indenter(case)
    rng = np.random.RandomState(7)
    box = np.asarray(s["box"], dtype=np.float64)
    L = box[:, 1] - box[:, 0]
    cloud = box[:, 0] - L + 3.0 * L * rng.rand(4000, 3)
    worst = [0.0, 0.0]
    for x in (s["x"], cloud):
        f, sums = _host_indent_force(x, o, s["box"])
        t = ir.terms(x, o, s["box"])
        assert int(t["touched"].sum()) >= 8
        ef = float((np.abs(f - t["f"]) / np.maximum(1.0, np.abs(t["f"]))).max())
        want = np.concatenate([[t["energy"]], t["findent"]])
        es = float((np.abs(sums - want) / np.maximum(1.0, np.abs(want))).max())
        worst = [max(worst[0], ef), max(worst[1], es)]
        assert np.array_equal(f != 0, np.broadcast_to(t["touched"][:, None], f.shape) & (t["f"] != 0))
    print("%-16s forces %.2e sums %.2e" % (case, worst[0], worst[1]))
    assert worst[0] < RUN0_BOUND and worst[1] < RUN0_BOUND


@pytest.mark.parametrize("case", list(ind.A_CASES))
def test_reference_against_recorded_run0(case):
    """indent_reference against what the reference binary computed at `run 0`: the indenter's share of every bead's force (recorded
    f with the indenter minus recorded f without), f_ID and f_ID[1..3] in both rows, pe without and with fix_modify energy yes.
    Bound 1e-12 relative to max(1, |value|); measured: at most 5.3e-15 (forces), 3.4e-15 (sums)."""
    fx, s = ind.a_fixture(), ind.a_system()
    n = len(s["x"])
    t = ir.terms(s["x"], ind.a_indenter(case), s["box"], ind.a_member(case))
    f, rows = fx["f_" + case], fx["rows_" + case]
    err = float((np.abs((f - fx["f0"]) - t["f"].astype(np.float64)) / np.maximum(1.0, np.abs(f))).max())
    print("%s: indenter force %.2e" % (case, err))
    assert err < RUN0_BOUND
    want = np.concatenate([[t["energy"]], t["findent"]]).astype(np.float64) / n          # (thermo_modify norm yes: per atom)
    for row in rows:
        assert (np.abs(row[2:] - want) <= RUN0_BOUND * np.maximum(1.0, np.abs(want))).all(), (row[2:], want)
    pe0 = float(fx["pe0"])
    assert rows[0][1] == pe0
    assert abs(rows[1][1] - (pe0 + want[0])) <= RUN0_BOUND * max(1.0, abs(pe0 + want[0]))


def test_conditions_on_the_run0_cases():
    assert len(ind.A_CASES) == 12
    for case in ind.A_CASES:
        assert ind.a_conditions(case) == "", case
    m = ind.meta()["a"]
    assert m["reference_operation_order"] < RUN0_BOUND and m["reference_sums"] < RUN0_BOUND


@pytest.mark.parametrize("name", ind.NAMES)
def test_conditions_on_the_recorded_runs(name):
    fx = ind.fixture(name)
    assert ind.fixture_conditions(fx) == ""
    assert fx.last <= 60 and len(fx.system()["x"]) <= 1000
    # the start touches the indenter too (f_c of the set-up row is not zero)
    assert ind.touched_fraction(fx.scn, fx.system()["x"], fx.system()["type"], 0) > 0


def test_conditions_on_the_recorded_minimisation():
    assert ind.c_conditions(ind.c_fixture()) == ""


@pytest.mark.skipif(not os.path.isfile(LMP), reason="oracle/_ref/lmp is not built here (no reference tree)")
@pytest.mark.parametrize("what", ["a", "shrink"])
def test_regeneration(tmp_path, what):
    """One fixture of each kind made again by the generator, into a directory of its own: the same numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_indent_runs as mk
    out = str(tmp_path)
    assert mk.main([what], out=out) == 0
    name = "indent_a.npz" if what == "a" else "indent_b_%s.npz" % what
    with np.load(os.path.join(out, name)) as new, np.load(os.path.join(ind.GOLDEN, name)) as old:
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), k
