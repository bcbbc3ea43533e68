"""fix spring/self, fix addforce and fix setforce without a device: grammar, error strings and refusals through the C-ABI, the
order rule and the capacity limit, fix_modify, the step plan with these fixes against the instantiations of the step kernel
(test hook lammps_le_test_step_plan_ext; nothing is launched), the origins through a restart file, the long-double restatement
(extforce_reference.py) against the recorded `run 0` of the reference binary, the conditions the fixtures were made under, and
- where the reference binary has been built - the regeneration of one fixture of each kind."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

import extforce_reference as er
import extforce_runs as ex
from systems import CHAIN_SCRIPT, lattice_chain, write_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")
# the factor of the recorded runs (reference_runs.FACTOR, what the wall tests hold their 48-step runs to) on the figures the
# generator wrote down for the long-double restatement against the reference's own operation order
FACTOR = 16.0


def _open(tmp_path, n=125, script=CHAIN_SCRIPT):
    from lammps_le_amd import lammps
    path = os.path.join(str(tmp_path), "data.chain")
    s = lattice_chain(n)
    s["image"][4] = (1, -2, 0)
    write_data(path, s)
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in script.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp, s


def _refuser(lmp):
    from lammps_le_amd import LammpsError

    def refused(line, text):
        with pytest.raises(LammpsError, match=text):
            lmp.command(line)
    return refused


def test_grammar_and_error_strings(tmp_path):
    lmp, _ = _open(tmp_path)
    refused = _refuser(lmp)
    for st in ("spring/self", "addforce", "setforce"):
        assert lmp.has_style("fix", st)
    lmp.command("fix 1 all nve")
    lmp.command("group some id 1:50:5")
    lmp.command("region box block 0 3 0 3 0 3")
    lmp.command("variable fx equal 1.0")
    # src/fix_spring_self.cpp:38-39, :48, :67
    refused("fix s some spring/self", "Illegal fix spring/self command")
    refused("fix s some spring/self 1.0 xyz 3", "Illegal fix spring/self command")
    refused("fix s some spring/self 0.0", "Illegal fix spring/self command")
    refused("fix s some spring/self -2.0", "Illegal fix spring/self command")
    refused("fix s some spring/self 1.0 zx", "Illegal fix spring/self command")
    refused("fix s nobody spring/self 1.0", "Could not find fix group ID")
    for k, word in enumerate(("xyz", "xy", "xz", "yz", "x", "y", "z")):
        lmp.command("fix t%d some spring/self 2.0 %s" % (k, word))
        lmp.command("unfix t%d" % k)
    # src/fix_addforce.cpp:42, :90-92, :109, :111
    refused("fix a some addforce 1.0 2.0", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 every", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 every 0", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 every -3", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 sometimes 3", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 energy 4.0", "Illegal fix addforce command")
    refused("fix a some addforce 1.0 2.0 3.0 region nowhere", "Region ID for fix addforce does not exist")
    # src/fix_setforce.cpp:40, :98
    refused("fix z some setforce 0 0", "Illegal fix setforce command")
    refused("fix z some setforce 0 0 0 every 2", "Illegal fix setforce command")
    refused("fix z some setforce 0 0 0 region nowhere", "Region ID for fix setforce does not exist")
    # what this engine refuses by name
    refused("fix a some addforce v_fx 0 0", "MI355X engine: fix addforce with a variable force")
    refused("fix a some addforce 0 0 v_fa", "MI355X engine: fix addforce with a variable force")
    refused("fix z some setforce v_fx NULL 0", "MI355X engine: fix setforce with a variable force")
    refused("fix z some setforce NULL NULL v_fa", "MI355X engine: fix setforce with a variable force")
    refused("fix a some addforce 1 2 3 region box", "MI355X engine: fix addforce with the region keyword")
    refused("fix z some setforce 0 0 0 region box", "MI355X engine: fix setforce with the region keyword")
    # energy v_name with constant components: the reference's words, at run (FixAddForce::init, :199-201)
    lmp.command("fix a some addforce 1.0 2.0 3.0 every 2 energy v_fx")
    refused("run 0", "Cannot use variable energy with constant force in fix addforce")
    lmp.command("unfix a")
    lmp.command("fix a some addforce 1.0 2.0 3.0 energy v_nosuch")
    refused("run 0", "Variable name for fix addforce does not exist")
    lmp.command("unfix a")
    # setforce under r-RESPA acts on every level: refused at run; spring/self and addforce are not
    lmp.command("fix z some setforce 0 NULL 0")
    lmp.command("run_style respa 2 2")
    refused("run 0", "MI355X engine: fix setforce under run_style respa")
    lmp.close()


def test_fix_modify_on_each_style(tmp_path):
    lmp, _ = _open(tmp_path)
    refused = _refuser(lmp)
    for line in ("fix 1 all nve", "fix s all spring/self 1.0", "fix a all addforce 0 0 1", "fix z all setforce NULL 0 NULL"):
        lmp.command(line)
    lmp.command("fix_modify s energy yes")
    lmp.command("fix_modify s energy no virial no")
    refused("fix_modify s virial yes", "Illegal fix_modify command")          # no virial_flag in spring/self
    lmp.command("fix_modify a energy yes virial yes")
    lmp.command("fix_modify a virial no")
    lmp.command("fix_modify z energy no virial no")
    refused("fix_modify z energy yes", "Illegal fix_modify command")          # setforce has neither
    refused("fix_modify z virial yes", "Illegal fix_modify command")
    for fid in "saz":
        refused("fix_modify %s energy maybe" % fid, "Illegal fix_modify command")
        refused("fix_modify %s energy" % fid, "Illegal fix_modify command")
        refused("fix_modify %s temp mine" % fid, "Illegal fix_modify command")
        refused("fix_modify %s respa 1" % fid, "MI355X engine: fix_modify respa is not supported")
    lmp.close()


def test_outputs_through_the_fix_virtuals(tmp_path):
    """Thermo columns, variable formulas and extract_fix reach the new scalars and vectors with no code of their own."""
    from lammps_le_amd import LammpsError
    lmp, _ = _open(tmp_path)
    refused = _refuser(lmp)
    for line in ("fix 1 all nve", "fix s all spring/self 1.0", "fix a all addforce 0 0 1", "fix z all setforce NULL 0 NULL"):
        lmp.command(line)
    lmp.command("thermo_style custom step pe f_s f_a f_a[1] f_a[3] f_z[1] f_z[3]")
    lmp.command("variable e equal f_s+f_a+f_a[2]+f_z[3]")
    assert lmp.extract_fix("s", 0, 0) == 0.0 and lmp.extract_fix("a", 0, 0) == 0.0
    assert lmp.extract_fix("a", 0, 1, 2) == 0.0 and lmp.extract_fix("z", 0, 1, 0) == 0.0
    with pytest.raises(LammpsError, match="out-of-range"):
        lmp.extract_fix("z", 0, 1, 3)
    with pytest.raises(LammpsError):
        lmp.extract_fix("s", 0, 1, 0)                      # spring/self has no vector
    lmp.command("variable bad equal f_a[4]")
    refused("print ${bad}", "Variable formula fix vector is accessed out-of-range")
    lmp.close()


def test_order_rule_and_the_ninth_fix(tmp_path):
    lmp, _ = _open(tmp_path)
    refused = _refuser(lmp)
    lmp.command("fix 1 all nve")
    lmp.command("region ball sphere 3 3 3 20.0 side in")
    # addforce / setforce ahead of a wall on the same side of fix langevin: refused at run, the message says what to do
    lmp.command("fix a all addforce 0 0 1")
    lmp.command("fix w all wall/region ball harmonic 1 1 1.1")
    refused("run 0", "define the wall first")
    lmp.command("unfix a")
    lmp.command("fix z all setforce 0 0 0")
    lmp.command("unfix w")
    lmp.command("fix w all wall/region ball harmonic 1 1 1.1")
    refused("run 0", "define the wall first")
    # on the other side of fix langevin the rule does not apply; spring/self may stand anywhere - these pass the rule and end
    # at the device, which this machine may not have
    lmp.command("unfix w")
    lmp.command("unfix z")
    lmp.command("fix s all spring/self 1.0")
    lmp.command("fix w all wall/region ball harmonic 1 1 1.1")
    lmp.command("fix a all addforce 0 0 1")
    lmp.command("fix 2 all langevin 1.0 1.0 1.0 4711")
    lmp.command("fix w2 all wall/region ball harmonic 1 1 1.1")
    lmp.command("fix z all setforce 0 0 0")
    from lammps_le_amd import LammpsError
    try:
        lmp.command("run 0")
    except LammpsError as e:
        assert "define the wall first" not in str(e)
    # FORCEOP_MAX = 8
    for k in range(5):
        lmp.command("fix m%d all addforce 0 0 %d" % (k, k))
    assert len([i for i in lmp.available_ids("fix") if i[0] in "sazm"]) == 8
    for line in ("fix n all spring/self 1.0", "fix n all addforce 0 0 1", "fix n all setforce 0 0 0"):
        refused(line, r"at most 8 fix spring/self, addforce and setforce instances \(FORCEOP_MAX")
    lmp.command("unfix m4")
    lmp.command("fix n all setforce 0 0 0")
    lmp.close()


# ------------------------------------------------------------------------------------------------------------------
# the step plan
# ------------------------------------------------------------------------------------------------------------------
def _hooks():
    from lammps_le_amd import library_path
    lib = ctypes.CDLL(library_path())
    out = []
    for name, nreq, nout in (("lammps_le_test_step_plan_soft", 13, 19), ("lammps_le_test_step_plan_ext", 14, 21)):
        fn = getattr(lib, name)
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        fn.restype = None

        def plan(n, dd, r, fn=fn, nreq=nreq, nout=nout):
            req, res = (ctypes.c_int * nreq)(*r), (ctypes.c_int * nout)()
            fn(n, dd, req, res)
            return list(res)
        out.append(plan)
    return out


SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_STEP_LDS_PAD", "LAMMPS_LE_DIAG_STEP")


@pytest.mark.parametrize("env", [{}, {"LAMMPS_LE_LPB": "1"}, {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}, {"LAMMPS_LE_NO_FUSE": "1"},
                                 {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0", "LAMMPS_LE_DIAG_STEP": "8"}])
def test_step_plan_with_the_fixes(monkeypatch, env):
    """Every request: without the fixes the new hook answers as the one before it; with them a fused plan names an
    instantiation the dispatcher holds, is the plan without them in everything but the flag, never takes velocities a rebuild
    left behind and never comes with the diagnostic launch; thermo steps, angle styles, fix nve / langevin on a group, walls,
    pair_style soft and runs without a pair style come back unfused.  Over the requests exactly 24 shapes fuse."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    old, new = _hooks()
    shapes = set()
    for n, dd in itertools.product((1000, 50001, 1000000), (0, 1)):
        for L, N, I, P, angles, thermo, check, cells in itertools.product((0, 1), repeat=8):
            for nvebit, lgbit, which in ((1, 1, -1), (2, 1, -1), (1, 2, -1), (1, 1, 1)):
                for walls, soft in ((0, 0), (1, 0), (2, 0), (0, 1)):
                    r = [L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells, walls, soft]
                    base = old(n, dd, r)
                    assert new(n, dd, r + [0])[:19] == base and new(n, dd, r + [0])[19] == 0
                    w = new(n, dd, r + [1])
                    if thermo or angles or not P or nvebit != 1 or lgbit != 1 or walls or soft or "LAMMPS_LE_NO_FUSE" in env:
                        assert w[0] == 0, (r, w)
                        continue
                    assert w[0] == 1 and w[19] == 1 and w[15] == 1, (r, w)          # fused, EXT, the dispatcher holds it
                    assert w[1:13] == base[1:13] and w[14] == base[14], (r, w, base)  # the same shape as without the fixes
                    assert w[13] == 0 and w[17] == 0, (r, w)                         # no diagnostic launch, no velocity hand-over
                    assert w[8] == w[9] == w[10] == w[6] == w[16] == w[18] == 0      # no ANG, EF, GRP, DIAG, WALL, SOFT with EXT
                    shapes.add(tuple(w[1:8]))                                        # langevin next ident pair lpb diag ahead
    if "LAMMPS_LE_NO_FUSE" in env:
        assert not shapes
    elif not env:
        assert len(shapes) == 24, sorted(shapes)      # L, N, I x {four lanes + look-ahead, one lane + look-ahead, throughput}
        assert {(s[4], s[6]) for s in shapes} == {(4, 1), (1, 1), (1, 0)} and all(s[3] == 1 and s[5] == 0 for s in shapes)


def test_count_of_step_variants():
    """count_step_variants(), as the built library states it through the hook: 129 before, 24 EXT variants more."""
    _, new = _hooks()
    assert new(1000, 0, [1, 1, 1, 1, 0, 0, 1, 1, -1, 0, 0, 0, 0, 1])[20] == 153


# ------------------------------------------------------------------------------------------------------------------
# restart
# ------------------------------------------------------------------------------------------------------------------
def _origins_via_restart(lmp, tmp_path, name):
    path = os.path.join(str(tmp_path), name)
    lmp.command("write_restart " + path)
    return path


def test_restart_round_trip_old_file_and_inconsistent_file(tmp_path):
    from lammps_le_amd import LammpsError, lammps
    lmp, s = _open(tmp_path)
    lmp.command("fix 1 all nve")
    lmp.command("group some id 1:50:5")
    plain = _origins_via_restart(lmp, tmp_path, "plain.restart")          # no spring/self: the layout of a file from before
    lmp.command("fix s some spring/self 3.0")
    # the origin is the position at the fix command: move the members afterwards, the file must carry the first positions
    lmp.command("set group some x 1.25")
    lmp.command("fix s2 all spring/self 1.0 xy")
    with_s = _origins_via_restart(lmp, tmp_path, "with.restart")
    lmp.close()
    assert os.path.getsize(with_s) > os.path.getsize(plain)
    raw = open(with_s, "rb").read()
    assert b"SPRINGSELF" in raw and b"SPRINGSELF" not in open(plain, "rb").read()
    # the origins of `s` as doubles, somewhere in the file: bead 1 (a member, index 0) with its unwrapped start position
    box = np.asarray(s["box"])
    prd = box[:, 1] - box[:, 0]
    want = np.zeros((len(s["x"]), 3))
    member = er.members(len(s["x"]), range(1, 51, 5))
    want[member] = (s["x"] + s["image"] * prd[None, :])[member]
    assert want.tobytes() in raw
    # bead 5 carries image flags (1, -2, 0) and is no member of `some`; it is one of `all`: s2 unwraps it
    moved = s["x"].copy()
    moved[member, 0] = 1.25
    want2 = moved + s["image"] * prd[None, :]
    assert want2.tobytes() in raw and s["image"][4].any()
    # a new handle: read_restart, the same fix commands -> the same origins in the next file (not the positions of now)
    b = lammps(cmdargs=["-screen", "none"])
    b.command("read_restart " + with_s)
    for ln in CHAIN_SCRIPT.split("\n"):
        if ln.split()[:1] and ln.split()[0] in ("neighbor", "neigh_modify", "comm_modify", "bond_style", "bond_coeff", "pair_style", "pair_modify", "pair_coeff"):
            b.command(ln)
    b.command("set group some x 2.5")
    b.command("fix s some spring/self 3.0")
    b.command("fix s2 all spring/self 1.0 xy")
    again = _origins_via_restart(b, tmp_path, "again.restart")
    raw2 = open(again, "rb").read()
    assert want.tobytes() in raw2 and want2.tobytes() in raw2
    # a fix of another ID takes nothing from the file
    b.command("fix s3 some spring/self 3.0")
    third = open(_origins_via_restart(b, tmp_path, "third.restart"), "rb").read()
    now = np.zeros_like(want)
    x_now = s["x"].copy()
    x_now[member, 0] = 2.5
    now[member] = (x_now + s["image"] * prd[None, :])[member]
    assert now.tobytes() in third
    b.close()
    # a file written before this change still reads
    c = lammps(cmdargs=["-screen", "none"])
    c.command("read_restart " + plain)
    c.command("fix s some spring/self 3.0")
    c.close()
    # the new section with a size that does not match natoms
    k = raw.index(want.tobytes())
    size_at = k - 8
    assert int.from_bytes(raw[size_at:k], "little") == want.size
    bad = raw[:size_at] + (want.size - 3).to_bytes(8, "little") + raw[k:k + want.nbytes - 24] + raw[k + want.nbytes:]
    bad_path = os.path.join(str(tmp_path), "bad.restart")
    open(bad_path, "wb").write(bad)
    d = lammps(cmdargs=["-screen", "none"])
    with pytest.raises(LammpsError, match="Restart file is inconsistent"):
        d.command("read_restart " + bad_path)
    d.close()


# ------------------------------------------------------------------------------------------------------------------
# the long-double restatement and the fixtures
# ------------------------------------------------------------------------------------------------------------------
def _rel(got, want):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def test_reference_against_recorded_run0():
    """extforce_reference from the recorded forces without the fixes against what the reference binary computed with them:
    per-bead forces, the fixes' thermo columns, their share of pe and press.  The figures are the ones the generator wrote
    into extforce_runs.json (recomputed here, they must be those), and they are rounding-sized: below 1e-13."""
    fx, m = ex.a_fixture(), ex.meta()["a"]
    ref_f, cols, pe, press = ex.a_reference(fx["f0"])
    dev_f = _rel(ref_f, fx["f"])
    k = ex.A_THERMO.index("f_s")
    dev_row = max(_rel(cols, fx["row"][k:]), _rel(pe, fx["row"][1] - fx["row0"][1]), _rel(press, fx["row"][2] - fx["row0"][2]))
    print("forces %.2e (recorded figure %.2e), row %.2e (%.2e)" % (dev_f, m["reference_operation_order"], dev_row, m["reference_sums"]))
    assert dev_f == m["reference_operation_order"] and dev_row == m["reference_sums"]
    assert 0 < dev_f < 1e-13 and 0 < dev_row < 1e-13


def test_conditions_on_the_run0_fixture():
    fx = ex.a_fixture()
    assert ex.a_conditions(fx["f"], fx["f0"]) == ""
    s = ex.a_system()
    box = np.asarray(s["box"])
    assert len(s["x"]) == 400 and 36 <= ex.a_members()["s"].sum() <= 44
    assert (box[:, 1] - box[:, 0]).min() >= 3 * (1.12 + 0.4)
    # no spring has zero length
    moved = np.abs(ex.a_positions() - s["x"]).max(axis=1)
    assert (moved[ex.a_members()["s"] | ex.a_members()["s2"]] > 0.03).all()
    x = ex.a_positions()
    assert (x >= box[:, 0]).all() and (x < box[:, 1]).all()


@pytest.mark.parametrize("name", ex.NAMES)
def test_conditions_on_the_recorded_runs(name):
    fx = ex.fixture(name)
    assert ex.fixture_conditions(fx) == ""
    assert fx.last == 48 and len(fx.system()["x"]) == 2048
    if name == "crossing":
        c = fx.meta["crossing"]
        assert 0 < c["flag_changed_at"] < 48 and c["builds_after_change"] > 0
        assert "group cross id %d\n" % c["bead"] in fx.scn["script"]


@pytest.mark.skipif(not os.path.isfile(LMP), reason="oracle/_ref/lmp is not built here (no reference tree)")
@pytest.mark.parametrize("what", ["a", "tether_behind"])
def test_regeneration(tmp_path, what):
    """One fixture of each kind made again by the generator, into a directory of its own: the same numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_extforce_runs as mk
    out = str(tmp_path)
    assert mk.main([what], out=out) == 0
    name = "extforce_a.npz" if what == "a" else "extforce_b_%s.npz" % what
    with np.load(os.path.join(out, name)) as new, np.load(os.path.join(ex.GOLDEN, name)) as old:
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), k
