"""The state the LE fixes leave behind on the device, against references that know nothing of the fixes (le_state.py).

Every LE parity test compares the engine with the CPU oracle, a restatement of the same reference statements by the same hands.
WHICH bonds the fixes move, create and break stays with the oracle (the bond multiset is compared with it here too); what
follows from the bonds is checked independently of it:
 (a) after runs that end on a quiet step, on an extrusion step and on a loading step: the invariants of the bond, special and
     angle tables (breadth-first search over the gathered bonds; the angle rule where no extruder moves), and f and the
     thermo keywords against force_reference.System built from the engine's OWN gathered topology at its own gathered
     positions - one evaluation, bound 16 x the oracle's deviation on the same input, at most 1e-12 (force_compare.bound);
 (b) the neighbor list of the last build entry by entry (test_gpu_neigh.check_list): bond records against the gathered
     tables, special codes against the search over the current bonds;
 (c) 24 steps through eleven table changes against a long-double trajectory whose topology follows the oracle's integer
     schedule, under the default switches, in the throughput shape of the step kernel and without the step kernel;
 (d) (a) on two z slabs;
 (e) a handle whose fixes move from a group to `all` (and back) between two runs against a fresh handle: bit for bit.
Nothing in any bound is derived from the engine's output.  The inputs, their conditions and the oracle's deviations are
asserted without a GPU in test_le_state_cpu.py."""
import numpy as np
import pytest

import force_compare as fc
import force_inputs as fi
import le_state as ls
from neigh_reference import delta
from neigh_worker import fetch_list
from systems import run_product
from test_gpu_force import PLAIN, STATS, report

pytestmark = pytest.mark.gpu
CASES = [(name, steps) for name in ls.NAMES if name != "levels-slab" for steps in ls.LENGTHS]
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO", "LAMMPS_LE_NO_FUSED_BIN",
            "LAMMPS_LE_NO_FUSED_GROUPS")


def check_end_state(label, name, steps, st, script, special_asym, fene_warnings):
    """(a) on a gathered state."""
    head, weights, barriers, fids, atype = ls.INPUTS[name]
    s = ls.system_of(name)
    bonds, angles = ls.check_state(st, weights)
    assert special_asym == 0 and fene_warnings == 0
    ost = ls.oracle_end(name, steps)[1]
    assert bonds == ls.check_bonds(ost), "the bond multiset is not the oracle's"
    assert np.array_equal(st.types, ost.types)
    if atype and "loop" not in fids:
        assert angles == ls.angle_rule(s, bonds, atype) and max(angles.values()) == 1
    S = ls.reference_for(script, s, bonds, angles, st.types)
    ev = S.evaluate(st.x)
    assert float(ev.gap) > delta(S.box, S.cutmax) and ev.fene_clamped == []
    odev = ls.oracle_reference(name, steps)[2]
    dev = ls.deviations(S, ev, st)
    bad = []
    for k in ("f",) + ls.KEYWORDS:
        b = fc.bound(odev[k], fc.RUN0_CEILING)
        print("%-24s %-6s engine %.2e  oracle %.2e  bound %.2e" % (label, k, dev[k], odev[k], b))
        if not dev[k] < b:
            bad.append("%s %s: %.3e exceeds %.3e (oracle %.3e)" % (label, k, dev[k], b, odev[k]))
    print("%-24s f per component: engine %.2e  oracle %.2e" % (label, dev["f_each"], odev["f_each"]))
    assert not bad, "\n".join(bad)
    return bonds, angles


@pytest.mark.parametrize("name,steps", CASES)
def test_end_state(tmp_path, name, steps):
    """(a).  Oracle figures (test_le_state_cpu.py): 12 - 34 extruder bonds, 18 - 52 unloads and 5 - 9 nonzero firings per fix at the
    end; on `levels` 245 / 303 / 251 pairs within the cutoff carry a level the data file does not give them (barriers 155 /
    194 / 170); oracle forces 2.5e-15 to 6.2e-15 of the largest force component, keywords at most 4.4e-15: every bound is the
    floor 1e-13.
    Measured on an MI355X: forces 2.8e-15 to 6.7e-15 of the largest component (per component 1.3e-13 to 8.7e-13, the oracle
    1.3e-13 to 9.5e-13: the engine rounds the separation of a pair across a face as the oracle does), keywords at most 3.8e-15."""
    script = ls.script_of(name, steps)
    p = run_product(script, ls.system_of(name), tmp_path)
    check_end_state("%s %d" % (name, steps), name, steps, ls.engine_state(p), script, p.stat("special_asym"), p.stat("fene_warnings"))
    assert p.stat("neigh_builds") == ls.oracle_end(name, steps)[0].neigh_builds()
    p.close()


@pytest.mark.parametrize("name,steps", [(name, steps) for name in ("wca-fene", "levels") for steps in ls.LENGTHS])
def test_list_after_firings(tmp_path, name, steps):
    """(b): the list of the last build of a run through ~25 firings.  Its positions are the current ones exactly when the last
    step rebuilt (the oracle tells: one step fewer, one build fewer); no pair of theirs is undecided (asserted in check_list)."""
    from test_gpu_neigh import FENE, check_list
    weights = FENE if name == "wca-fene" else (ls.LEVELS_W, (0.0, 0.0, 0.0))
    s = ls.system_of(name)
    p = run_product(ls.script_of(name, steps), s, tmp_path)
    st = ls.engine_state(p)
    bonds = ls.check_bonds(st)
    assert any(b[0] == ls.EXTRUDER for b in bonds) and bonds != sorted(tuple(b) for b in s["bonds"].tolist())
    L = fetch_list(p)
    x, ref = check_list(L, s, (st.num_bond, st.bond_type, st.bond_atom), p.stat("neigh_pairs"), weights, bonds=bonds,
                        cutneigh=ls.cutoff_of(name) + 0.4)
    builds = ls.oracle_end(name, steps)[0].neigh_builds()
    on_last_step = ls.oracle_end(name, steps - 1)[0].neigh_builds() != builds
    assert p.stat("neigh_builds") == builds and p.stat("special_asym") == 0
    assert np.array_equal(x, st.x) == on_last_step, "build positions %s the current ones" % ("are not" if on_last_step else "are")
    if name == "levels":
        codes = np.bincount(L["code"], minlength=4)
        print("codes", codes)
        assert codes[1] == 0 and codes[2] > 500 and codes[3] > 500
    p.close()


VARIANTS = {"default": {}, "plain": PLAIN, "unfused": {"LAMMPS_LE_NO_FUSE": "1"}}
PATHS = {"default": dict(steps_fused=ls.K - 3, steps_unfused=3), "plain": dict(steps_fused=ls.K - 3, steps_fused_thermo=3),
         "unfused": dict(steps_unfused=ls.K)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["levels", "angles-all"])
def test_trajectory_through_firings(tmp_path, monkeypatch, name, variant):
    """(c): 24 steps from a relaxed start, extrusion every 4, ex_load every 5, ex_unload every 6 steps, `thermo 8`.  The end
    bond and angle multisets are the schedule's last entry; then x (unwrapped), v, f after the last step and every thermo row
    against the reference trajectory, and x and v after each of the steps 1 .. 23 from fresh runs, each under 16 x the
    deviation of an oracle run of as many steps (ceilings 1e-9 x, 1e-8 v and f, 1e-9 rows).
    Oracle deviations (levels / angles-all): x 4.0e-15 / 4.3e-15, v 1.1e-13 / 1.1e-13, f 2.9e-12 / 4.8e-12, rows 5.7e-15 / 6.7e-15; after
    the steps 1 .. 23 x at most 5.0e-15, v 1.4e-13.
    Measured on an MI355X, the three variants alike: x 4.0e-15 / 4.3e-15 (bound 1.0e-13), v 1.2e-13 / 1.1e-13 (1.7e-12 / 1.8e-12),
    f 3.3e-12 / 4.8e-12 (4.6e-11 / 7.7e-11), rows 5.3e-15 / 6.7e-15 (1.0e-13 / 1.1e-13); after the steps 1 .. 23 x equal to the oracle's
    deviation in every printed digit, v within 1.1 of it; 21 of the 24 steps through the step kernel."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in VARIANTS[variant].items():
        monkeypatch.setenv(k, val)
    s = ls.system_of(name, True)
    weights = ls.INPUTS[name][1]
    p = run_product(ls.traj_script(name), s, tmp_path)
    stats = {k: int(p.stat(k)) for k in STATS}
    print(name, variant, stats)
    x, v, f, image, rows = p.gather("x"), p.gather("v"), p.gather("f"), p.gather("image"), p.thermo_history()
    st = ls.engine_state(p)
    assert ls.check_state(st, weights) == ls.schedule(name)[-1], "the end topology is not the schedule's last entry"
    assert p.stat("special_asym") == 0 and p.stat("fene_warnings") == 0
    builds = p.stat("neigh_builds")
    p.close()
    # the path: the three thermo steps (8, 16, 24) through the energy variant where the shape has one (the throughput shape,
    # without angles) and through the unfused kernels elsewhere, every other step - the thirteen on which a fix fires among
    # them - through the step kernel: otherwise this test would say nothing about it
    assert stats == dict(dict.fromkeys(STATS, 0), **PATHS[variant if (variant, name) != ("plain", "angles-all") else "default"]), stats
    S, ref = ls.reference_trajectory(name)
    last, states, obuilds = ls.oracle_trajectory(name)
    assert float(min(ref["gaps"])) > ls.traj_required_gap(name)
    label = "%s %s" % (name, variant)
    bad = report(label + " x", S.unwrapped(x, image), ref["x"][-1], last["x"], fc.TRAJ_CEILING["x"])
    bad += report(label + " v", v, ref["v"][-1], last["v"], fc.TRAJ_CEILING["v"])
    bad += report(label + " f", f, ref["f"], last["f"], fc.TRAJ_CEILING["f"])
    steps = list(range(0, ls.K + 1, ls.TRAJ_THERMO))
    assert [int(r[0]) for r in rows] == steps, rows[:, 0]
    want = [[ref["rows"][k][key] for key in fc.ROW_KEYS] for k in steps]
    bad += report(label + " thermo rows", rows[:, 1:6], want, last["rows"], fc.TRAJ_CEILING["rows"])
    assert [int(r[6]) for r in rows] == [len(ls.schedule(name)[k][0]) for k in steps]
    assert not bad, "\n".join(bad)
    assert builds == obuilds, (builds, obuilds)
    for k in range(1, ls.K):
        p = run_product(ls.traj_script(name, k), s, tmp_path)
        bad += report("%s x after step %d" % (label, k), S.unwrapped(p.gather("x"), p.gather("image")), ref["x"][k], states[k - 1]["x"],
                      fc.TRAJ_CEILING["x"])
        bad += report("%s v after step %d" % (label, k), p.gather("v"), ref["v"][k], states[k - 1]["v"], fc.TRAJ_CEILING["v"])
        assert ls.check_bonds(ls.engine_state(p)) == ls.schedule(name)[k][0], "bonds after step %d" % k
        p.close()
    assert not bad, "\n".join(bad)


def test_decomposed(tmp_path):
    """(d): `levels` in a box stretched along z to four ghost cutoffs of 3.5, on two slabs (threads of this process over the
    in-process transport): the checks of (a) on the joined state after 121 steps.  Measured on an MI355X: forces 6.9e-15 of
    the largest component (oracle 3.8e-15, bound 1.0e-13)."""
    from test_gpu_dd import run_ranks_local
    name, steps = "levels-slab", ls.LENGTHS[1]
    script = ls.script_of(name, steps)

    def extra(lmp):
        return dict(state=ls.engine_state(lmp), ranks=lmp.stat("comm_nranks"), nlocal=lmp.stat("nlocal"), asym=lmp.stat("special_asym"),
                    fene=lmp.stat("fene_warnings"))
    r = run_ranks_local(2, ls.system_of(name), script, tmp_path, extra=extra)
    assert r["ranks"] == 2 and 50 < r["nlocal"] < 550
    check_end_state("2 slabs", name, steps, r["state"], script, r["asym"], r["fene"])
    assert int(r["builds"][0]) == ls.oracle_end(name, steps)[0].neigh_builds()


# ------------------------------------------------------------------------------------------------
# (e) state that outlives a run command on one handle
# ------------------------------------------------------------------------------------------------
GROUPED = "group mobile type 1\nfix 1 mobile nve\nfix 2 mobile langevin 1.0 1.0 1.0 %d\n"
ON_ALL = "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 %d\n"


@pytest.mark.parametrize("order", ["grouped-then-all", "all-then-grouped"])
def test_fixes_change_their_group_between_runs(tmp_path, order):
    """`offset-pinned` (every seventh bead of type 2): fix nve and fix langevin on the type-1 beads for 20 steps, unfix both, the
    same fixes on `all` with another seed for 20 steps - and the reverse order - against a fresh handle that reads the state
    after the first run from a restart file (written by a third handle, so that nothing touches the handle under test
    between its runs) and runs the second part alone: x, v and f bit for bit.  What travels with an upload (the masks, the
    rank of every bead among the thermostat's members, their count, which cuts the random stream into calls) must follow
    the fixes, also when the last fix on a group goes."""
    from lammps_le_amd import lammps
    case = fi.INPUTS["offset-pinned"]()
    head = fi.script(case, skin="0.2")
    first, second = (GROUPED % 48611, ON_ALL % 90217) if order == "grouped-then-all" else (ON_ALL % 48611, GROUPED % 90217)
    second = "unfix 1\nunfix 2\n" + second + "run 20\n"
    rfile = str(tmp_path / "after_first.restart")
    w = run_product(head + first + "thermo 10\nrun 20\nwrite_restart %s\n" % rfile, case["system"], tmp_path)
    w.close()
    a = run_product(head + first + "thermo 10\nrun 20\n", case["system"], tmp_path)
    mid, mid_image = a.gather("x"), a.gather("image")
    for ln in second.split("\n"):
        a.command(ln)
    b = lammps(cmdargs=["-screen", "none"])
    b.command("read_restart " + rfile)
    assert np.array_equal(b.gather("x"), mid)          # (the restart is the state the handle under test continues from)
    for ln in ("thermo 10\n" + second.replace("unfix 1\nunfix 2\n", "")).split("\n"):
        b.command(ln)
    pinned = case["system"]["type"] == 2
    assert pinned.sum() == 90
    # (unwrapped: a bead that left the box during the first run is wrapped by the setup of the second)
    prd = np.asarray(case["system"]["box"])[:, 1] - np.asarray(case["system"]["box"])[:, 0]
    moved = np.abs((a.gather("x") + a.gather("image") * prd) - (mid + mid_image * prd)).max(axis=1) > 1e-9
    if order == "grouped-then-all":
        assert moved.all()
    else:
        assert not moved[pinned].any() and moved[~pinned].all()
    for k in ("x", "v", "f", "image"):
        assert np.array_equal(a.gather(k), b.gather(k)), "%s differs from the fresh handle's by %.3e" % (k, np.abs(a.gather(k) - b.gather(k)).max())
    a.close(), b.close()
