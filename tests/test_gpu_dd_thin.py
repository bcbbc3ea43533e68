"""Decomposed runs on slabs between ONE and TWO ghost cutoffs thick (csrc/device.h slab_rule): a bead can lie within the
ghost cutoff of both faces of its slab and is then in both send lists (k_dd_borders, DeviceState::sendboth).  Every halo
path - staging buffer filled by the step kernel, pack kernel, overlap mode, peer windows in both launch forms, verify
mode, receive buffer + unpack - against the one-rank CPU oracle, with the tolerances the thick-slab tests of
test_gpu_dd.py use for the same comparisons.  Each test asserts that its slabs really are thinner than two ghost cutoffs.

Geometry (density 0.85, lattice spacing 1.0557): 20000 beads -> box 29.56, 27000 -> 31.67, 60000 -> 42.23, 100000 -> 49.62."""
import os
import threading
import time
import uuid

import numpy as np
import pytest

from systems import CHAIN_SCRIPT, lattice_chain, run_oracle, write_data
from test_gpu_dd import bond_set, run_ranks, run_ranks_local
from test_gpu_le import LE, barrier_types, melted, special_sets

pytestmark = pytest.mark.gpu
MD = "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nthermo 30\nrun 60\n"
STATS = ("halo_sent_both", "halo_pack_launches", "nlocal", "nghost", "neigh_builds")


def thin(system, world, cutghost):
    """Slab width; asserts cutghost <= w < 2 * cutghost, i.e. the case the two-cutoff rule refused."""
    box = np.asarray(system["box"], dtype=np.float64)
    w = (box[2, 1] - box[2, 0]) / world
    assert cutghost <= w < 2.0 * cutghost, (w, cutghost)
    assert w + 2.0 * cutghost <= box[2, 1] - box[2, 0]
    return w


def run_ranks_stats(world, system, script, tmp_path, expect_error=None):
    """run_ranks_local of test_gpu_dd.py (ranks = threads of this process, in-process transport) that also returns the
    per-rank counters of STATS from every rank.  expect_error: every rank's script must end in an error with this text
    (returned: the messages); the handles must still close."""
    from lammps_le_amd import lammps
    session = uuid.uuid4().hex[:12]
    path = os.path.join(str(tmp_path), "data.local")
    write_data(path, system)
    out, stats, errs, msgs = [None] * world, [None] * world, [], [None] * world

    def work(rank):
        try:
            lmp = lammps(cmdargs=["-screen", "none"])
            lmp.comm_init("local", rank, world, session=session)
            try:
                for ln in script.split("\n"):
                    w = ln.split("#")[0].split()
                    lmp.command("read_data " + path if w and w[0] == "read_data" else ln)
            except Exception as e:
                if expect_error is None:
                    raise
                msgs[rank] = str(e)
                lmp.close()
                return
            stats[rank] = {k: lmp.stat(k) for k in STATS}
            res = dict(x=lmp.gather("x"), v=lmp.gather("v"), image=lmp.gather("image"),
                       num_bond=lmp.gather("num_bond"), bond_type=lmp.gather("bond_type"), bond_atom=lmp.gather("bond_atom"),
                       nspecial=lmp.gather("nspecial"), special=lmp.gather("special"),
                       thermo=np.array([lmp.get_thermo(k) for k in ("temp", "epair", "emol", "etotal", "press", "bonds")]),
                       neigh_pairs=np.array([lmp.stat("neigh_pairs")]), builds=np.array([lmp.stat("neigh_builds")]))
            if lmp.extract_setting("angle_per_atom") > 0:
                res.update(num_angle=lmp.gather("num_angle"), angle_type=lmp.gather("angle_type"), angle_atom1=lmp.gather("angle_atom1"),
                           angle_atom2=lmp.gather("angle_atom2"), angle_atom3=lmp.gather("angle_atom3"),
                           nangles=np.array([lmp.extract_setting("nangles")]))
            for fid in ("loop", "loading", "unloading"):
                try:
                    res["f_" + fid] = np.array([lmp.extract_fix(fid, 0, 1, 0), lmp.extract_fix(fid, 0, 1, 1)])
                except Exception:
                    pass
            out[rank] = res
            lmp.close()
        except Exception as e:       # a failing rank leaves the others waiting for the transport's timeout
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    if expect_error is not None:
        return msgs
    for r in range(1, world):        # every rank holds the same gathered state
        assert np.array_equal(out[r]["x"], out[0]["x"]) and np.array_equal(out[r]["bond_atom"], out[0]["bond_atom"])
    return out[0], stats


def assert_md(r, o):
    """the assertions of test_md_across_slabs_in_process"""
    assert np.abs(r["x"] - o.x()).max() < 1e-9
    assert np.abs(r["v"] - o.v()).max() < 1e-8
    assert (r["image"] == o.image()).all()
    assert np.abs(r["thermo"][:5] - o.thermo()[:5]).max() < 1e-9
    assert r["neigh_pairs"][0] == 2 * o.neigh_pairs()
    assert r["builds"][0] == o.neigh_builds()


def assert_le(r, o):
    """the assertions of test_le_fixes_across_three_slabs_in_process"""
    assert bond_set(r["num_bond"], r["bond_type"], r["bond_atom"]) == o.bond_set()
    ns_o, sp_o = o.special_table()
    assert special_sets(r["nspecial"], r["special"]) == special_sets(ns_o, sp_o)
    for fid in ("loop", "loading", "unloading"):
        assert r["f_" + fid][0] == o.fix_vector(fid)[0] and r["f_" + fid][1] == o.fix_vector(fid)[1]
    assert np.abs(r["x"] - o.x()).max() < 1e-7


# ---- 1: plain MD, the recommended script as it is -----------------------------------------------------------------------
@pytest.mark.parametrize("world,overlap", [(4, 0), (5, 0), (4, 1), (5, 1)])
def test_md_on_thin_slabs_with_the_recommended_cutoff(tmp_path, world, overlap, monkeypatch):
    """CHAIN_SCRIPT with its `comm_modify cutoff 5.0` left in, 20000 beads (box 29.56): 4 slabs of 7.39, 5 of 5.91.  Only a
    far-shell bead with a bond partner on another rank is sent beyond the pair shell, and a lattice start has none that
    reaches both sides: no bead is in both lists, and the halo still comes out of the step kernel (no pack launch per step)."""
    monkeypatch.setenv("LAMMPS_LE_OVERLAP", str(overlap))
    s = lattice_chain(20000, nchains=2, seed=23)
    thin(s, world, 5.0)
    assert "comm_modify cutoff 5.0" in CHAIN_SCRIPT
    script = CHAIN_SCRIPT + MD
    o = run_oracle(script, s)
    r, stats = run_ranks_stats(world, s, script, tmp_path)
    print("halo_sent_both", [st["halo_sent_both"] for st in stats], "halo_pack_launches", [st["halo_pack_launches"] for st in stats],
          "builds", int(o.neigh_builds()))
    assert_md(r, o)
    for st in stats:
        assert st["halo_sent_both"] == 0
        # k_dd_pack runs only for a halo whose positions did not come out of the fused step kernel: the steps that rebuild do
        # not pack at all (k_dd_pack_xt), what is left are the first step and the steps behind a thermo evaluation
        assert 0 <= st["halo_pack_launches"] <= int(o.neigh_builds()) + 5, st


# ---- 2: whole-shell ghosts: most beads of a slab are in both lists ------------------------------------------------------
def semiflexible_case(style):
    from test_gpu_angle import ANGLE_SCRIPT, semiflexible
    s = semiflexible(27000, 3, seed=4, steps=300)
    coeffs = ("angle_coeff 1 1.5 160.0", "angle_coeff 2 1.0 100.0") if style == "harmonic" else ("angle_coeff 1 1.5", "angle_coeff 2 0.5")
    script = ANGLE_SCRIPT.replace("bond_coeff 2 5.0 10.0 1.0 1.0", "bond_coeff 2 8.0 5.0 1.0 1.0") + """angle_style %s
%s
%s
fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
fix loop all extrusion 19 1 1 1 1.0 2
fix loading all ex_load 5 1 1 1.12 2 prob 0.3 684474 iparam 1 1 jparam 1 1 atype 2
fix unloading all ex_unload 6 2 0.5 prob 0.4 456456
thermo 20
run 50
""" % ((style,) + coeffs)
    assert "comm_modify cutoff 5.0" in script
    return s, script


@pytest.mark.parametrize("style", ["harmonic", "cosine"])
def test_semiflexible_chains_on_thin_slabs(tmp_path, style):
    """The scenario of test_semiflexible_chains_across_slabs on 4 slabs of 7.92 (box 31.67, ghost cutoff 5.0).  A run with an
    angle style ghosts the whole shell, so every bead with 2.92 <= z - slab_lo < 5.0 is in both lists: a quarter of a slab."""
    s, script = semiflexible_case(style)
    thin(s, 4, 5.0)
    o = run_oracle(script, s)
    r, stats = run_ranks_stats(4, s, script, tmp_path)
    print("halo_sent_both", [st["halo_sent_both"] for st in stats], "nlocal", [st["nlocal"] for st in stats])
    assert all(st["halo_sent_both"] > 0 for st in stats)
    assert any(st["halo_sent_both"] >= 0.1 * st["nlocal"] for st in stats)
    assert bond_set(r["num_bond"], r["bond_type"], r["bond_atom"]) == o.bond_set()
    na, at, a1, a2, a3 = o.angle_table()
    assert (r["num_angle"] == na).all()
    for name, ref in (("angle_type", at), ("angle_atom1", a1), ("angle_atom2", a2), ("angle_atom3", a3)):
        for i in np.nonzero(na)[0]:
            assert list(r[name][i, :na[i]]) == list(ref[i, :na[i]]), (name, i + 1)
    assert int(r["nangles"][0]) == o.nangles()
    assert any(a[0] == 2 for a in o.angle_set())
    for fid in ("loop", "loading", "unloading"):
        assert r["f_" + fid][0] == o.fix_vector(fid)[0] and r["f_" + fid][1] == o.fix_vector(fid)[1]
    assert np.abs(r["x"] - o.x()).max() < 1e-8
    assert np.abs(r["thermo"][:5] - o.thermo()[:5]).max() < 1e-8
    assert r["builds"][0] == o.neigh_builds()


# ---- 3: LE fixes with long extruder bonds -------------------------------------------------------------------------------
def le_case(sort=False, rows_along_z=False):
    """rows_along_z: the same melt with its x and z axes exchanged (the box is cubic).  lattice_chain lays a chain in rows along
    x, 1600 beads to a z layer, and 1500 steps of melting leave that order in place: an extruder bond, which joins beads a few
    places apart on one row, then spans up to 6 in x and never more than 1.7 in z, too little to reach from one face of an 8.45
    slab to within 6.2 of the other.  With the rows along z it spans up to 4.5 in z."""
    n = 60000
    s = melted(n, nchains=3, seed=9, types=barrier_types(n, 17))
    if rows_along_z:
        for k in ("x", "v", "image"):
            s[k] = np.ascontiguousarray(np.asarray(s[k])[:, ::-1])
    base = CHAIN_SCRIPT.replace("comm_modify cutoff 5.0", "comm_modify cutoff 6.2") \
        .replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 10.0 6.0 1.0 1.0")
    if sort:
        base = base.replace("atom_modify sort 0 0", "atom_modify sort 5 0")
    return s, base + LE.format(n1=20, nl=10, nu=10, neutral=1, left=2, right=3, tp=0.5, lr="4",
                               lprob="prob 0.5 684474", uprob="prob 0.3 456456", rmax=0.5) + "run 50\n"


def both_list_beads(x, system, world, cutpair, cutghost, bonds):
    """What k_dd_borders would put into both send lists at positions x: per rank, the beads within the ghost cutoff of both
    faces that are in the pair shell of a face or have a bond partner on another rank (bond-based ghost shell)."""
    box = np.asarray(system["box"], dtype=np.float64)
    lo, prd = box[2, 0], box[2, 1] - box[2, 0]
    w = prd / world
    z = (x[:, 2] - lo) % prd
    owner = np.minimum((z / w).astype(int), world - 1)
    zc = z - owner * w
    remote = np.zeros(len(x), dtype=bool)
    for _, a, b in bonds:
        if owner[a - 1] != owner[b - 1]:
            remote[a - 1] = remote[b - 1] = True
    dn = (zc < cutpair) | ((zc < cutghost) & remote)
    up = (zc >= w - cutpair) | ((zc >= w - cutghost) & remote)
    return np.bincount(owner[dn & up], minlength=world)


@pytest.mark.parametrize("world", [5, 6])
def test_le_fixes_on_thin_slabs(tmp_path, world):
    """The scenario of test_le_fixes_across_three_slabs_in_process (ghost cutoff 6.2, extruder bonds up to 6.0 long, box
    42.23) on 5 slabs of 8.45 and 6 of 7.04, the chains' rows along z (le_case).  A bead bonded across a face and within 6.2 of
    the other face is in both lists: at the oracle's final positions 8 beads on 5 slabs, some 1500 on 6."""
    s, script = le_case(rows_along_z=True)
    thin(s, world, 6.2)
    o = run_oracle(script, s)
    expect = both_list_beads(o.x(), s, world, 1.52, 6.2, o.bond_set())
    print("both-list beads at the oracle's final positions, per rank:", expect.tolist())
    assert expect.sum() > 0          # (known without a device: the scenario does hold such beads)
    r, stats = run_ranks_stats(world, s, script, tmp_path)
    print("halo_sent_both", [st["halo_sent_both"] for st in stats])
    assert_le(r, o)
    assert sum(st["halo_sent_both"] for st in stats) > 0


# ---- 4: eight slabs at 100k ---------------------------------------------------------------------------------------------
def test_eight_thin_slabs_with_the_bench_script(tmp_path):
    """test_eight_slabs_with_the_bench_script at 100000 beads: eight slabs of 6.20 under `comm_modify cutoff 5.0`."""
    from lammps_le_amd.synth import CHAIN_INPUT, lattice_chains
    from systems import OracleScript
    n = 100000
    sysd = lattice_chains(n, nchains=1, seed=3, barrier_every=200)
    script = CHAIN_INPUT.format(data="data.chain", n1=10, left=2, right=3, tp=0.5, lr="4", nload=10, pload=0.2, punload=0.2) + "run 34\n"
    assert "comm_modify cutoff 5.0" in script
    thin(sysd, 8, 5.0)
    osc = OracleScript(dict(sysd))
    for ln in script.split("\n"):
        if not ln.startswith("thermo_style"):
            osc.line(ln)
    o = osc.o
    r = run_ranks_local(8, sysd, script.replace("thermo_style", "#thermo_style"), tmp_path)
    assert bond_set(r["num_bond"], r["bond_type"], r["bond_atom"]) == o.bond_set()
    assert len([b for b in o.bond_set() if b[0] == 2]) > 10
    for fid in ("loop", "loading", "unloading"):
        assert r["f_" + fid][0] == o.fix_vector(fid)[0] and r["f_" + fid][1] == o.fix_vector(fid)[1]
    assert np.abs(r["x"] - o.x()).max() < 1e-7 and (r["image"] == o.image()).all()
    assert r["builds"][0] == o.neigh_builds() and r["neigh_pairs"][0] == 2 * o.neigh_pairs()


# ---- 5: peer windows and transports, one process per rank ---------------------------------------------------------------
@pytest.mark.parametrize("windows", [1, 2, 0])
def test_md_on_thin_slabs_one_process_per_rank(tmp_path, windows, monkeypatch):
    """Case 1's system on 4 ranks in four processes: the per-step halo through the peer windows in the two-launch and the
    one-launch form, every window halo also sent through the transport and compared (verify mode), and once with the
    windows off."""
    monkeypatch.setenv("LAMMPS_LE_OVERLAP", "0")
    monkeypatch.setenv("LAMMPS_LE_FAST_HALO", str(min(windows, 1)))
    monkeypatch.setenv("LAMMPS_LE_HALO_FUSED", "1" if windows == 2 else "0")
    monkeypatch.setenv("LAMMPS_LE_FAST_HALO_VERIFY", "1" if windows else "0")
    s = lattice_chain(20000, nchains=2, seed=23)
    thin(s, 4, 5.0)
    script = CHAIN_SCRIPT + MD
    o = run_oracle(script, s)
    r = run_ranks(4, s, script, tmp_path)
    assert_md(r, o)
    nwin = int(r["window_exchanges"][0])
    print("window_exchanges", nwin, "window_mismatches", int(r["window_mismatches"][0]))
    if windows:
        assert 60 - int(o.neigh_builds()) - 5 <= nwin <= 60, nwin
        assert int(r["window_mismatches"][0]) == 0
    else:
        assert nwin == 0


def test_whole_shell_ghosts_through_verified_windows(tmp_path, monkeypatch):
    """Case 2's scenario in four processes with windows + verify: beads in both lists go through the step kernel's stores into
    both neighbours' windows, and every ghost is compared with the transport's copy of the same halo."""
    monkeypatch.setenv("LAMMPS_LE_OVERLAP", "0")
    monkeypatch.setenv("LAMMPS_LE_FAST_HALO", "1")
    monkeypatch.setenv("LAMMPS_LE_HALO_FUSED", "0")
    monkeypatch.setenv("LAMMPS_LE_FAST_HALO_VERIFY", "1")
    s, script = semiflexible_case("harmonic")
    thin(s, 4, 5.0)
    o = run_oracle(script, s)
    r = run_ranks(4, s, script, tmp_path)
    assert bond_set(r["num_bond"], r["bond_type"], r["bond_atom"]) == o.bond_set()
    for fid in ("loop", "loading", "unloading"):
        assert r["f_" + fid][0] == o.fix_vector(fid)[0] and r["f_" + fid][1] == o.fix_vector(fid)[1]
    assert np.abs(r["x"] - o.x()).max() < 1e-8
    assert np.abs(r["thermo"][:5] - o.thermo()[:5]).max() < 1e-8
    assert r["builds"][0] == o.neigh_builds()
    print("window_exchanges", int(r["window_exchanges"][0]), "window_mismatches", int(r["window_mismatches"][0]))
    assert int(r["window_exchanges"][0]) > 0 and int(r["window_mismatches"][0]) == 0


# ---- 6: the list itself -------------------------------------------------------------------------------------------------
def test_neighbor_list_on_thin_slabs(tmp_path):
    """The decomposed case of test_gpu_neigh.py on 5 slabs of 6.33 (box 31.67, `comm_modify cutoff 5.0`): every rank's device
    list, entry by entry, against brute force."""
    import neigh_inputs as I
    from test_gpu_neigh import FENE, check_list, joined, run_in_children
    s, meta = I.slab_ladder()
    thin(s, 5, 5.0)
    assert "comm_modify cutoff 5.0" in I.ZERO_SCRIPT
    ranks = run_in_children(5, s, I.ZERO_SCRIPT + "run 0\n", tmp_path)
    assert all(len(r["owned"]) > 0 for r in ranks)
    r0 = ranks[0]
    assert sum(len(r["itag"]) for r in ranks) == r0["neigh_pairs"][0]
    check_list(joined(ranks), s, (r0["num_bond"], r0["bond_type"], r0["bond_atom"]), r0["neigh_pairs"][0], FENE, r0["x"])


# ---- 7: other modes -----------------------------------------------------------------------------------------------------
def test_le_fixes_on_thin_slabs_under_atom_sort(tmp_path):
    """test_le_fixes_across_slabs_under_atom_sort on 5 slabs of 8.45 (ghost cutoff 6.2)."""
    s, script = le_case(sort=True)
    thin(s, 5, 6.2)
    o = run_oracle(script, s)
    r = run_ranks_local(5, s, script, tmp_path)
    assert bond_set(r["num_bond"], r["bond_type"], r["bond_atom"]) == o.bond_set()
    for fid in ("loop", "loading", "unloading"):
        assert r["f_" + fid][0] == o.fix_vector(fid)[0] and r["f_" + fid][1] == o.fix_vector(fid)[1]
    assert np.abs(r["x"] - o.x()).max() < 1e-7
    o0 = run_oracle(script.replace("atom_modify sort 5 0", "atom_modify sort 0 0"), s)
    assert o0.bond_set() != o.bond_set()


def test_respa_on_thin_slabs(tmp_path):
    """test_respa_across_slabs (three levels, bond 1 pair 2) on 4 slabs of 7.39 with the recommended cutoff 5.0."""
    s = lattice_chain(20000, nchains=2, seed=21, jitter=0.03)
    thin(s, 4, 5.0)
    script = CHAIN_SCRIPT + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nrun_style respa 3 2 3 bond 1 pair 2\nthermo 20\nrun 40\nrun 20\n"
    o = run_oracle(script, s)
    r = run_ranks_local(4, s, script, tmp_path)
    assert np.abs(r["x"] - o.x()).max() < 1e-8
    assert np.abs(r["v"] - o.v()).max() < 1e-7
    assert (r["image"] == o.image()).all()
    assert np.abs(r["thermo"][:5] - o.thermo()[:5]).max() < 1e-8
    assert r["builds"][0] == o.neigh_builds()


def test_fixes_on_a_group_on_thin_slabs(tmp_path):
    """The langevin-subset case of test_md_fixes_on_groups_across_slabs on 4 slabs of 7.39 with the recommended cutoff 5.0."""
    n = 20000
    types = 1 + (np.arange(n) % 7 == 0).astype(np.int32)
    s = lattice_chain(n, nchains=2, seed=29, jitter=0.03, types=types)
    s["mass"] = [1.0, 1.0]
    thin(s, 4, 5.0)
    body = "group hot id 1:%d:3 %d:%d\nfix 1 all nve\nfix 2 hot langevin 1.2 0.8 2.0 91 scale 2 2.5\n" % (n // 2, n // 2 + 100, n)
    script = CHAIN_SCRIPT + body + "thermo 20\nrun 45\nrun 25\n"
    o = run_oracle(script, s)
    r = run_ranks_local(4, s, script, tmp_path)
    assert np.abs(r["x"] - o.x()).max() < 1e-9
    assert np.abs(r["v"] - o.v()).max() < 1e-8
    assert (r["image"] == o.image()).all()
    assert np.abs(r["thermo"][:5] - o.thermo()[:5]).max() < 1e-9
    assert r["builds"][0] == o.neigh_builds()


def test_md_on_thin_slabs_without_direct_receive(tmp_path, monkeypatch):
    """LAMMPS_LE_NO_DIRECT_RECV=1 (read at every run command; one process per rank all the same): the halo lands in the receive
    buffer and an unpack kernel scatters it; the send lists keep the order k_dd_borders gave them."""
    monkeypatch.setenv("LAMMPS_LE_NO_DIRECT_RECV", "1")
    monkeypatch.setenv("LAMMPS_LE_OVERLAP", "0")
    monkeypatch.setenv("LAMMPS_LE_FAST_HALO_VERIFY", "0")
    s = lattice_chain(20000, nchains=2, seed=23)
    thin(s, 4, 5.0)
    script = CHAIN_SCRIPT + MD
    o = run_oracle(script, s)
    r = run_ranks(4, s, script, tmp_path)
    assert_md(r, o)
    assert int(r["window_exchanges"][0]) == 0          # (the windows need the receiver's sorted order)
    import rebuild_rules as R
    plan = int(r["rebuild_plan"][0])                   # the last rebuild: decomposed, no reorder of the send lists
    assert not plan & R.DIRECT_RECV and (plan & R.DDCODE) >> R.DDCODE_SHIFT == 1 and not plan & (R.PREBINNED | R.WRAP_BIN)


# ---- 8: still refused ---------------------------------------------------------------------------------------------------
def test_a_slab_below_one_ghost_cutoff_is_refused_on_every_rank(tmp_path, monkeypatch):
    """6 ranks on the 20000-bead box (w = 4.93 < 5.0): every rank raises the width error before anything collective starts,
    so no rank waits for another - the test ends well inside the communicator's time-out - and every handle still closes."""
    monkeypatch.setenv("LAMMPS_LE_COMM_TIMEOUT", "30")
    s = lattice_chain(20000, nchains=2, seed=23)
    box = np.asarray(s["box"])
    assert (box[2, 1] - box[2, 0]) / 6 < 5.0
    t0 = time.time()
    msgs = run_ranks_stats(6, s, CHAIN_SCRIPT + MD, tmp_path, expect_error="one ghost cutoff")
    took = time.time() - t0
    assert all(m is not None and "slab thinner than one ghost cutoff" in m for m in msgs), msgs
    assert took < 30, took
