"""fix wall/region without a device: the script layer's error strings through the C-ABI, the step plan with walls against the
instantiations of the step kernel (test hook lammps_le_test_step_plan_walls; nothing is launched), the long-double wall
reference (wall_reference.py) against the recorded `run 0` fixtures of the reference binary, and the conditions those fixtures
and the recorded runs inside the sphere were made under (wall_runs.py)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import wall_reference as wr
import wall_runs as wl
from systems import CHAIN_SCRIPT, lattice_chain, write_data

# the project's bound for single evaluations against reference-held vectors, relative to max(1, |f|)
RUN0_BOUND = 1e-12


def _open(tmp_path, n=125):
    from lammps_le_amd import lammps
    path = os.path.join(str(tmp_path), "data.chain")
    write_data(path, lattice_chain(n))
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in CHAIN_SCRIPT.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp


def test_script_layer(tmp_path):
    from lammps_le_amd import LammpsError
    lmp = _open(tmp_path)
    assert lmp.has_style("fix", "wall/region")
    for line in ("region ball sphere 3 3 3 9.0 side in", "region hole sphere 3 3 3 0.5 side out", "region box block -1 9 -1 9 -1 9",
                 "region pipe cylinder z 3 3 8 -1 9", "region pipe_out cylinder z 3 3 0.2 -1 9 side out", "region both union 2 ball box",
                 "region common intersect 2 ball box", "fix 1 all nve"):
        lmp.command(line)

    def refused(line, text):
        with pytest.raises(LammpsError, match=text):
            lmp.command(line)
    # src/fix_wall_region.cpp:39, :66, :71-72, :80-81: argument counts and the style name
    refused("fix w all wall/region ball lj126 1.0 1.0", "Illegal fix wall/region command")
    refused("fix w all wall/region ball lj126 1.0 1.0 1.1 7", "Illegal fix wall/region command")
    refused("fix w all wall/region ball morse 1.0 1.0 1.1", "Illegal fix wall/region command")
    refused("fix w all wall/region ball harmonic 1.0 1.0 1.1 2.0", "Illegal fix wall/region command")
    refused("fix w all wall/region ball table 1.0 1.0 1.1", "Illegal fix wall/region command")
    refused("fix w all wall/region nowhere lj126 1.0 1.0 1.1", "Region ID for fix wall/region does not exist")     # :53-55
    refused("fix w all wall/region ball lj93 1.0 1.0 0.0", r"Fix wall/region cutoff <= 0.0")                          # :88
    refused("fix w all wall/region ball morse 1.0 2.0 0.5 -1.0", r"Fix wall/region cutoff <= 0.0")
    refused("fix w all wall/region ball colloid 1.0 1.0 1.1", "Fix wall/region colloid requires atom style sphere")  # :127-128
    refused("fix w nobody wall/region ball lj126 1.0 1.0 1.1", "Could not find fix group ID")
    # regions whose contact sets the kernels do not restate: named in the message
    refused("fix w all wall/region pipe_out lj126 1.0 1.0 1.1", "does not support region style cylinder with side out")
    refused("fix w all wall/region both lj126 1.0 1.0 1.1", "does not support region style union")
    refused("fix w all wall/region common lj126 1.0 1.0 1.1", "does not support region style intersect")
    for k, (region, style) in enumerate((("ball", "lj93 1 1 1.1"), ("hole", "lj126 1 1 1.1"), ("box", "lj1043 1 1 1.1"), ("pipe", "morse 1 2 0.5 1.1"))):
        lmp.command("fix w%d all wall/region %s %s" % (k, region, style))
    refused("fix w4 all wall/region ball harmonic 1 1 1.1", "at most 4 fix wall/region")                 # WALL_MAX
    assert lmp.available_ids("fix") == ["1", "w0", "w1", "w2", "w3"]
    lmp.command("unfix w3")
    lmp.command("fix w4 all wall/region box harmonic 1 1 1.1")
    # fix_modify (src/fix.cpp:134-176)
    lmp.command("fix_modify w0 energy yes virial yes")
    lmp.command("fix_modify w0 energy no")
    refused("fix_modify w0 energy maybe", "Illegal fix_modify command")
    refused("fix_modify w0 energy", "Illegal fix_modify command")
    refused("fix_modify w0", "Illegal fix_modify command")
    refused("fix_modify w0 temp mine", "Illegal fix_modify command")
    refused("fix_modify 1 energy yes", "Illegal fix_modify command")
    refused("fix_modify 1 virial yes", "Illegal fix_modify command")
    refused("fix_modify nosuch energy yes", "Could not find fix_modify ID")
    refused("fix_modify w0 respa 1", "fix_modify respa is not supported")
    # f_ID and f_ID[1..3]; beyond that the reference's words (src/thermo.cpp:949, src/variable.cpp:1700)
    lmp.command("thermo_style custom step pe f_w0 f_w0[1] f_w0[3]")
    lmp.command("variable e equal f_w0+f_w0[2]")
    assert lmp.extract_fix("w0", 0, 0) == 0.0 and lmp.extract_fix("w0", 0, 1, 2) == 0.0
    lmp.command("variable bad equal f_w0[4]")
    refused("print ${bad}", "Variable formula fix vector is accessed out-of-range")
    with pytest.raises(LammpsError, match="out-of-range"):
        lmp.extract_fix("w0", 0, 1, 3)
    # the region can go between the command and a run: said again at the run (FixWallRegion::init)
    lmp.command("region box delete")
    refused("run 0", "Region ID for fix wall/region does not exist")
    lmp.close()


# ------------------------------------------------------------------------------------------------------------------
def _hooks():
    from lammps_le_amd import library_path
    lib = ctypes.CDLL(library_path())
    out = []
    for name, nreq, nout in (("lammps_le_test_step_plan", 11, 16), ("lammps_le_test_step_plan_walls", 12, 18)):
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
def test_step_plan_with_walls(monkeypatch, env):
    """Every request: without walls the new hook answers as the old one; with fusable walls a fused plan names an instantiation
    that exists, is the plan without walls in everything but the wall flag, never takes velocities a rebuild left behind and
    never comes with the diagnostic launch; thermo steps, angle styles, fixes on groups, runs without a pair style and walls on
    a group come back unfused."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    old, new = _hooks()
    fused_wall = 0
    for n, dd in itertools.product((1000, 50001, 1000000), (0, 1)):
        for L, N, I, P, angles, thermo, check, cells in itertools.product((0, 1), repeat=8):
            for nvebit, lgbit, which in ((1, 1, -1), (2, 1, -1), (1, 2, -1), (1, 1, 1)):
                r = [L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells]
                base = old(n, dd, r)
                assert new(n, dd, r + [0])[:16] == base and new(n, dd, r + [0])[16] == 0
                assert new(n, dd, r + [2])[0] == 0
                w = new(n, dd, r + [1])
                if thermo or angles or not P or nvebit != 1 or lgbit != 1 or "LAMMPS_LE_NO_FUSE" in env:
                    assert w[0] == 0, (r, w)
                    continue
                assert w[0] == 1 and w[16] == 1 and w[15] == 1, (r, w)          # fused, wall, the instantiation exists
                assert w[1:13] == base[1:13] and w[14] == base[14], (r, w, base)  # the same shape as without the wall
                assert w[13] == 0 and w[17] == 0, (r, w)                         # no diagnostic launch, no velocity hand-over
                assert w[8] == w[9] == w[10] == w[6] == 0                        # no ANG, EF, GRP, DIAG with WALL
                fused_wall += 1
    assert fused_wall > 0 or "LAMMPS_LE_NO_FUSE" in env


# ------------------------------------------------------------------------------------------------------------------
CASES = [(r, s) for r in wl.REGIONS for s in wl.STYLES]


@pytest.mark.parametrize("region,style", CASES)
def test_reference_against_recorded_run0(region, style):
    """wall_reference against what the reference binary computed at `run 0`: the wall's share of every bead's force
    (recorded f with the wall minus recorded f without), f_ID, f_ID[1..3], and the change of pe and press under fix_modify
    energy / virial yes.  Bound 1e-12 relative to max(1, |value|); measured: at most 2.9e-14 (sphere_in lj126, forces)."""
    fx = wl.a_fixture(region)
    s = wl.a_system()
    t = wr.wall_terms(s["x"], wr.parse_region(wl.REGIONS[region].split()), wr.parse_wall(wl.STYLES[style].split()))
    f, rows = fx["f_" + style], fx["rows_" + style]
    err = float((np.abs((f - fx["f0"]) - t["f"].astype(np.float64)) / np.maximum(1.0, np.abs(f))).max())
    print("%s %s: wall force %.2e" % (region, style, err))
    assert err < RUN0_BOUND
    col = wl.A_THERMO.index
    for row in rows:
        for k, name in enumerate(("f_w", "f_w[1]", "f_w[2]", "f_w[3]")):
            want = (float(t["energy"]) if k == 0 else float(t["fwall"][k - 1])) / len(s["x"])       # (thermo_modify norm yes: per atom)
            assert abs(row[col(name)] - want) <= RUN0_BOUND * max(1.0, abs(want)), (name, row[col(name)], want)
    n = len(s["x"])
    # fix_modify no: pe and press are those of the run without the wall; yes: + energy / N and + trace(virial) / (3 V)
    box = np.asarray(s["box"])
    vol = float(np.prod(box[:, 1] - box[:, 0]))
    pe0, press0 = fx["row0"][1], fx["row0"][2]
    assert rows[0][col("pe")] == pe0 and rows[0][col("press")] == press0
    pe1, press1 = pe0 + float(t["energy"]) / n, press0 + float(t["virial"][:3].sum()) / (3.0 * vol)
    assert abs(rows[1][col("pe")] - pe1) <= RUN0_BOUND * max(1.0, abs(pe1))
    assert abs(rows[1][col("press")] - press1) <= RUN0_BOUND * max(1.0, abs(press1))


def test_conditions_on_the_run0_fixtures():
    """Every block face and every cylinder surface (curved, both caps) has a contact, some bead has two block contacts at
    once, no bead is outside, for every style's cutoff; and the figure wall_runs.json holds for the reference's own operation
    order is below the bound."""
    s = wl.a_system()
    for region, style in CASES:
        reg = wr.parse_region(wl.REGIONS[region].split())
        t = wr.wall_terms(s["x"], reg, wr.parse_wall(wl.STYLES[style].split()))
        assert not t["outside"].any(), (region, style)
        assert len(t["faces"]) == {"sphere": 1, "block": 6 if reg["side"] == "in" else 1, "cylinder": 3}[reg["style"]]
        assert all(h.any() for h in t["faces"]), (region, style, [int(h.sum()) for h in t["faces"]])
        if region == "block_in":
            assert (t["ncontact"] >= 2).any() and (t["ncontact"] == 3).any()
    assert wl.meta()["a"]["reference_operation_order"]["value"] < RUN0_BOUND


def test_outside_and_on_the_surface_are_told():
    ball = dict(style="sphere", side="in", args=(0.0, 0.0, 0.0, 2.0))
    wall = wr.parse_wall("lj126 1.0 1.0 1.1".split())
    x = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [0.0, 2.0, 0.0], [2.5, 0.0, 0.0]])
    t = wr.wall_terms(x, ball, wall)
    assert list(t["outside"]) == [False, False, True, True] and list(t["ncontact"]) == [0, 1, 0, 0]
    assert t["f"][1, 2] < 0 and not t["f"][[0, 2, 3]].any()


@pytest.mark.parametrize("name", wl.NAMES)
def test_conditions_on_the_recorded_runs(name):
    """The LE fixes acted, extruder bonds exist, at least 5 % of the beads the wall acts on are within its cutoff at the
    recorded step, none is outside the sphere; the start is inside the sphere too."""
    fx = wl.fixture(name)
    assert wl.fixture_conditions(fx) == ""
    frac, out = wl.near_wall_fraction(fx.system()["x"])
    assert not out and frac >= 0.05
    assert fx.last <= 60 and len(fx.system()["x"]) <= 1000
