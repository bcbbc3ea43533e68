"""Forces, energies, virial, pressure and the integration of the HIP path against a long-double brute force.

Every other parity test of the force path compares the kernels with the CPU oracle - a restatement of the same statements by
the same hands in the same operation order.  Here the other side is tests/force_reference.py: plain numpy in long double,
from nothing but positions, velocities, types, masses, box, bonds, angles and the script's coefficients - no cells, no list,
no image words, no coefficient tables - and pinned to the reference program's own known answers without a GPU
(test_force_reference_cpu.py).  The inputs (force_inputs.py) put bonds and angles across all three pairs of faces at setup,
use cutoffs up to 2.5 without a shift, hubs of up to six bonds, free beads, a bead without neighbors, a clamped FENE bond,
an exactly straight angle, and wavefronts that lie wholly between half a cutoff and a cutoff from a face.

Bounds: for every compared quantity 16 x the deviation of the FP64 oracle from the reference on the same input (computed
here, force_compare.bound), at least 1e-13, never above the project's ceilings (1e-12 for a single evaluation; 1e-9 for x,
1e-8 for v and f, 1e-9 for thermo rows after twelve steps).  Nothing is derived from the engine's output.  The reference
needs no list: a missed or late rebuild shows as a force error.  The engine hands positions and velocities out at the end
of a run: the states after steps 1 .. 11 are those of fresh runs of 1 .. 11 steps from the same start (test_trajectory)."""
import numpy as np
import pytest

import force_compare as fc
import force_inputs as fi
from neigh_reference import delta
from systems import run_product

pytestmark = pytest.mark.gpu

RUN0 = ["tiny", "aligned", "offset", "types", "hubs", "hubs-harmonic", "angles-harmonic", "angles-cosine", "fene-large"]
PTENSOR = "thermo_style custom step temp epair emol etotal press pxx pyy pzz pxy pxz pyz\n"


def report(what, got, ref, oracle_dev, ceiling):
    err, b = fc.relerr(got, ref), fc.bound(oracle_dev, ceiling)
    print("%-28s engine %.2e  oracle %.2e  bound %.2e" % (what, err, oracle_dev, b))
    return [] if err < b else ["%s: %.3e exceeds %.3e (oracle %.3e)" % (what, err, b, oracle_dev)]


# ------------------------------------------------------------------------------------------------
# (a) one evaluation: k_force<EFLAG> (+ k_angle), k_ke_tensor, k_colsum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["yes", "no"])
@pytest.mark.parametrize("name", RUN0)
def test_run0(tmp_path, name, norm):
    """Per-bead forces and evdwl, ebond, eangle, pe, ke, temp, press, pxx .. pyz of `run 0` under thermo_modify norm yes | no;
    the bond-image path the engine took (stat bond_minimg: the per-step minimum image on fene-large, the frozen image words on
    every other input - tiny and offset are all-FENE too, in boxes too narrow for it); on hubs the FENE warning count against
    the one clamped bond.
    Measured on an MI355X (engine / oracle / bound, relative with floor 1): forces between 1.6e-14 / 1.6e-14 / 2.6e-13 (aligned)
    and 5.6e-14 / 4.6e-14 / 7.3e-13 (types); every thermo keyword at most 2.0e-15 (oracle: 8.5e-15) against bounds of 1.0e-13 to
    1.4e-13.  A halved interior margin does not show here, not even on aligned (the evaluation at setup does not see the
    wavefronts its zones are built for); it shows in test_trajectory[default-aligned] and [plain-aligned]."""
    case = fi.INPUTS[name]()
    S, x, v, img = fc.reference_system(name)
    ev = fc.reference_run0(name)
    dev, _ = fc.oracle_run0(name)
    p = run_product(fi.script(case, norm=norm) + PTENSOR + "run 0\n", case["system"], tmp_path)
    # the positions the engine used are the positions the reference used; no candidate pair of theirs is undecided
    assert np.array_equal(p.gather("x"), x) and np.array_equal(p.gather("image"), img)
    assert float(ev.gap) > delta(S.box, S.cutmax)
    bad = report(name + " f", p.gather("f"), ev.f, dev["f"], fc.RUN0_CEILING)
    ref = fc.thermo_of(name, ev, v, norm)
    for k in fc.THERMO_KEYS:
        bad += report("%s %s norm %s" % (name, k, norm), p.get_thermo(k), ref[k], dev[(k, norm)], fc.RUN0_CEILING)
    assert not bad, "\n".join(bad)
    assert p.stat("bond_minimg") == fi.BOND_MINIMG[name]
    assert p.stat("fene_warnings") == len(ev.fene_clamped) == (1 if name.startswith("hubs") else 0)
    p.close()


# ------------------------------------------------------------------------------------------------
# (b) twelve steps: the k_step variants and the unfused kernels
# ------------------------------------------------------------------------------------------------
PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
# id: (input, fixes, switches, thermo interval, steps by path).  Twelve steps with `thermo 4` have thermo steps 4, 8, 12: only
# the throughput shape has an energy variant of the step kernel, every other shape takes its thermo steps through the unfused
# kernels - `thermo 1` there would keep the step kernel from running at all.
TRAJ = {
    "default-tiny": ("tiny", "nve", {}, 4, dict(steps_fused=9, steps_unfused=3)),
    "default-aligned": ("aligned", "nve", {}, 4, dict(steps_fused=9, steps_unfused=3)),
    "plain-aligned": ("aligned", "nve", PLAIN, 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "default-hubs": ("hubs-harmonic", "nve", {}, 4, dict(steps_fused=9, steps_unfused=3)),
    "morse-hubs": ("hubs", "nve", {}, 4, dict(steps_unfused=12)),          # (bond morse: the unfused kernels, whatever the shape)
    "default-types": ("types", "nve", {}, 4, dict(steps_fused=9, steps_unfused=3)),
    "default-fene-large": ("fene-large", "nve", {}, 4, dict(steps_fused=9, steps_unfused=3)),
    "plain-offset": ("offset", "nve", PLAIN, 1, dict(steps_fused_thermo=12)),
    "plain-types": ("types", "nve", PLAIN, 1, dict(steps_fused_thermo=12)),
    "plain-offset-thermo4": ("offset", "nve", PLAIN, 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "plain-offset-unfused-thermo": ("offset", "nve", dict(PLAIN, LAMMPS_LE_NO_FUSED_THERMO="1"), 4, dict(steps_fused=9, steps_unfused=3)),
    "plain-offset-unfused-bin": ("offset", "nve", dict(PLAIN, LAMMPS_LE_NO_FUSED_BIN="1"), 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "plain-types-thermo4": ("types", "nve", PLAIN, 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "plain-types-unfused-thermo": ("types", "nve", dict(PLAIN, LAMMPS_LE_NO_FUSED_THERMO="1"), 4, dict(steps_fused=9, steps_unfused=3)),
    "plain-types-unfused-bin": ("types", "nve", dict(PLAIN, LAMMPS_LE_NO_FUSED_BIN="1"), 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "ahead-hubs": ("hubs-harmonic", "nve", AHEAD, 4, dict(steps_fused=9, steps_unfused=3)),
    "unfused-offset": ("offset", "nve", {"LAMMPS_LE_NO_FUSE": "1"}, 1, dict(steps_unfused=12)),
    "group-fused": ("offset-pinned", "group", {}, 4, dict(steps_fused=9, steps_fused_group=9, steps_unfused=3)),
    "group-unfused": ("offset-pinned", "group", {"LAMMPS_LE_NO_FUSED_GROUPS": "1"}, 4, dict(steps_unfused=12)),
    "angles-harmonic-plain": ("angles-harmonic", "nve", PLAIN, 4, dict(steps_fused=9, steps_unfused=3)),
    "angles-harmonic-ahead": ("angles-harmonic", "nve", AHEAD, 4, dict(steps_fused=9, steps_unfused=3)),
    "angles-cosine-plain": ("angles-cosine", "nve", PLAIN, 4, dict(steps_fused=9, steps_unfused=3)),
    "angles-cosine-ahead": ("angles-cosine", "nve", AHEAD, 4, dict(steps_fused=9, steps_unfused=3)),
    "langevin-plain": ("offset", "langevin", PLAIN, 1, dict(steps_fused_thermo=12)),
    "langevin-plain-thermo4": ("offset", "langevin", PLAIN, 4, dict(steps_fused=9, steps_fused_thermo=3)),
    "langevin-default": ("offset", "langevin", {}, 4, dict(steps_fused=9, steps_unfused=3)),
}
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused")


def compare_trajectory(label, name, fixes, thermo, x, v, image, f, rows, builds):
    S = fc.reference_system(name, fixes)[0]
    ref = fc.reference_trajectory(name, fixes)
    dev, obuilds = fc.oracle_trajectory(name, fixes)
    # no pair came closer to a cutoff than a hundred times what the position bound can move it
    assert float(min(ref["gaps"])) > fc.required_gap(name, fixes)
    bad = report(label + " x", S.unwrapped(x, image), ref["x"][-1], dev["x"], fc.TRAJ_CEILING["x"])
    bad += report(label + " v", v, ref["v"][-1], dev["v"], fc.TRAJ_CEILING["v"])
    bad += report(label + " f", f, ref["f"], dev["f"], fc.TRAJ_CEILING["f"])
    steps = list(range(0, fc.STEPS + 1, thermo))
    assert [int(r[0]) for r in rows] == steps, rows[:, 0]
    want = [[ref["rows"][k][key] for key in fc.ROW_KEYS] for k in steps]
    bad += report(label + " thermo rows", rows[:, 1:6], want, dev["rows"], fc.TRAJ_CEILING["rows"])
    assert not bad, "\n".join(bad)
    assert obuilds >= 3 and builds == obuilds, (builds, obuilds)


@pytest.mark.parametrize("case", sorted(TRAJ))
def test_trajectory(tmp_path, case, monkeypatch):
    """Twelve velocity-Verlet steps at temperature ~5 with neighbor 0.2 (three or four list builds): unwrapped positions,
    velocities and forces after the last step and every thermo row against the reference; the engine's list builds against the
    oracle's; the path the steps took.  Pinned beads keep their positions bit for bit.  Then the positions and velocities
    after each of the steps 1 .. 11, from fresh runs of as many steps under the same switches (the last step of a run is a
    thermo step, so the k-th step of these runs is the energy variant or the unfused kernels where the twelve-step run
    takes the plain one; the paths asserted are those of the twelve-step run), each under 16 x the deviation of an oracle
    run of as many steps.
    Measured on an MI355X (engine / oracle deviation from the reference, the largest over the cases): after the last step x
    3.6e-15 / 3.6e-15 (bound 1.0e-13), v 1.1e-12 / 1.1e-12 (bounds from 7.6e-13, on hubs, where both are at 5e-14), f 1.4e-11 /
    1.4e-11, thermo rows 4.6e-14 / 5.6e-14 (1.0e-13); after the steps 1 .. 11 x 3.0e-15 / 3.0e-15 (1.0e-13), v 1.3e-12 / 1.3e-12;
    on types in the throughput shape (thermo 1, thermo 4,
    separate thermo, separate binning alike) x 5.1e-16, v 1.4e-13, f 1.2e-12, rows at most 7.6e-15; on aligned (three rebuilds,
    the wavefronts still the zones) x 6.2e-16, v 6.3e-14, f 2.1e-12 (3.3e-11)."""
    name, fixes, env, thermo, paths = TRAJ[case]
    for k in ("LAMMPS_LE_LPB", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO", "LAMMPS_LE_NO_FUSED_BIN",
              "LAMMPS_LE_NO_FUSED_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    system = fi.INPUTS[name]()["system"]
    p = run_product(fc.run_script(name, fixes, thermo), system, tmp_path)
    stats = {k: int(p.stat(k)) for k in STATS}
    print(case, stats)
    compare_trajectory(case, name, fixes, thermo, p.gather("x"), p.gather("v"), p.gather("image"), p.gather("f"),
                       p.thermo_history(), p.stat("neigh_builds"))
    assert stats == dict(dict.fromkeys(STATS, 0), **paths), stats
    assert p.stat("bond_minimg") == fi.BOND_MINIMG[name]
    S, x0 = fc.reference_system(name, fixes)[:2]
    if fixes == "group":
        assert (~S.mobile).sum() == 90 and np.array_equal(p.gather("x")[~S.mobile], x0[~S.mobile])
    p.close()
    ref, odev, bad = fc.reference_trajectory(name, fixes), fc.oracle_states(name, fixes), []
    for k in range(1, fc.STEPS):
        p = run_product(fc.run_script(name, fixes, thermo, steps=k), system, tmp_path)
        bad += report("%s x after step %d" % (case, k), S.unwrapped(p.gather("x"), p.gather("image")), ref["x"][k], odev[k - 1]["x"],
                      fc.TRAJ_CEILING["x"])
        bad += report("%s v after step %d" % (case, k), p.gather("v"), ref["v"][k], odev[k - 1]["v"], fc.TRAJ_CEILING["v"])
        p.close()
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# (c) decomposed: z slabs on 2 and 3 ranks (threads of this process, in-process transport)
# ------------------------------------------------------------------------------------------------
def rank_results(lmp):
    """What test_gpu_dd.run_ranks_local returns of a rank on top of its own: forces, thermo keywords, rows, the steps' paths."""
    return dict(f=lmp.gather("f"), keywords={k: lmp.get_thermo(k) for k in fc.THERMO_KEYS[:7]}, rows=lmp.thermo_history(),
                ranks=lmp.stat("comm_nranks"), nlocal=lmp.stat("nlocal"), paths={k: int(lmp.stat(k)) for k in STATS})


@pytest.mark.parametrize("world", [2, 3])
def test_decomposed(tmp_path, world):
    """`offset` cut into 2 and 3 slabs along z (14.8 long; ghost cutoff 2.0), the ranks as threads over the in-process transport
    (test_gpu_dd.run_ranks_local; it keeps the halo off the peer windows, every exchange goes through the transport): the
    run-0 forces and thermo, then the twelve-step trajectory, against the same reference and under the same bounds as the
    single-GPU tests; nine steps through the step kernel, the three thermo steps through the unfused kernels (a decomposed
    run has no energy variant).  The states after steps 1 .. 11 are not compared here, by choice: the slabs run the step
    kernel test_trajectory compares step by step, and what is theirs alone - halo, migration, rebuilds - shows after the last.
    Measured on an MI355X (2 and 3 ranks alike): run-0 forces 5.1e-14 (bound 6.6e-13), press 1.3e-16; after twelve steps x 3.6e-15
    (1.0e-13), v 5.9e-13 (9.4e-12), f 8.8e-12 (1.4e-10), thermo rows 2.1e-14 (9.0e-13)."""
    from test_gpu_dd import run_ranks_local
    name = "offset"
    case = fi.INPUTS[name]()
    S, x, v, img = fc.reference_system(name)
    ev = fc.reference_run0(name)
    dev, _ = fc.oracle_run0(name)
    r0 = run_ranks_local(world, case["system"], fi.script(case, skin="0.2") + "run 0\n", tmp_path, extra=rank_results)
    assert r0["ranks"] == world and 0 < r0["nlocal"] < S.n and np.array_equal(r0["x"], x)
    bad = report("%d ranks f" % world, r0["f"], ev.f, dev["f"], fc.RUN0_CEILING)
    ref = fc.thermo_of(name, ev, v, "yes")
    for k in fc.THERMO_KEYS[:7]:
        bad += report("%d ranks %s" % (world, k), r0["keywords"][k], ref[k], dev[(k, "yes")], fc.RUN0_CEILING)
    assert not bad, "\n".join(bad)
    r1 = run_ranks_local(world, case["system"], fc.run_script(name, "nve", 4), tmp_path, extra=rank_results)
    compare_trajectory("%d ranks" % world, name, "nve", 4, r1["x"], r1["v"], r1["image"], r1["f"], r1["rows"], int(r1["builds"][0]))
    assert r1["ranks"] == world and r1["paths"] == dict(dict.fromkeys(STATS, 0), steps_fused=9, steps_unfused=3), r1["paths"]
