"""CPU tests of the local pair computes: the script layer (every accepted and refused command of compute property/local
natom* / patom* and compute pair/local, with the reference program's error strings), the refusal to answer before a run,
and - for the GPU tests of test_gpu_pair_rows.py - the two properties of their inputs that need no GPU: the NEIGH reference rows
(pair_rows_reference.py) are as many as the oracle's half list holds, and no state a GPU test compares holds a pair within
`neigh_reference.delta` of the cutoff that decides it."""
import os

import numpy as np
import pytest

import pair_rows_reference as PR
from lammps_le_amd import LMP_SIZE_ROWS, LMP_STYLE_LOCAL, LMP_TYPE_VECTOR, LammpsError, lammps
from systems import CHAIN_SCRIPT, lattice_chain, run_oracle, write_data


def _open(tmp_path, script=CHAIN_SCRIPT, n=500):
    s = lattice_chain(n)
    path = os.path.join(str(tmp_path), "data.chain")
    write_data(path, s)
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in script.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp


ACCEPTED = [
    "compute n1 all property/local natom1 natom2 ntype1 ntype2",
    "compute n2 all property/local natom2",
    "compute p1 all property/local patom1 patom2 ptype1 ptype2",
    "compute p2 all property/local ptype2 patom1 cutoff type",
    "compute b1 all property/local btype batom1 batom2",
    "compute d1 all pair/local dist",
    "compute d2 all pair/local dist eng force fx fy fz",
    "compute d3 all pair/local eng fz cutoff type",
    "compute d4 odd pair/local force",
    "compute x1 all pair/local dist p1 p3",          # refused at the run: lj/cut has no extra fields
]
REFUSED = [
    ("compute r1 all property/local natom1 patom2", "Compute property/local cannot use these inputs together"),
    ("compute r2 all property/local batom1 natom2", "Compute property/local cannot use these inputs together"),
    ("compute r3 all property/local ptype1 btype", "Compute property/local cannot use these inputs together"),
    ("compute r4 all property/local natom1 cutoff radius", "Compute property/local requires atom attribute radius"),
    ("compute r5 all property/local natom1 cutoff", "Illegal compute property/local command"),
    ("compute r6 all property/local natom1 frobnicate", "Illegal compute property/local command"),
    ("compute r7 all property/local", "Illegal compute property/local command"),
    ("compute r8 all pair/local", "Illegal compute pair/local command"),
    ("compute r9 all pair/local dist cutoff radius", "Compute pair/local requires atom attribute radius"),
    ("compute r10 all pair/local dist px", "Invalid keyword in compute pair/local command"),
    ("compute r11 all pair/local dist p0", "Invalid keyword in compute pair/local command"),
    ("compute r12 all pair/local dist cutoff", "Illegal compute pair/local command"),
    ("compute r13 all pair/local dist cutoff sphere", "Illegal compute pair/local command"),
    ("compute r14 all pair/local dist frobnicate", "Illegal compute pair/local command"),      # compute_pair_local.cpp:65, 82
    ("compute r15 nobody pair/local dist", "Could not find compute group ID"),
    ("compute r16 all contact/local dist", "Unknown compute style contact/local"),
]


def test_commands_accepted_and_refused(tmp_path):
    """(a) argument grammar and error strings of the reference's constructors, the style and ID lists, dump local columns."""
    lmp = _open(tmp_path)
    lmp.command("group odd id 1:499:2")
    for cmd in ACCEPTED:
        lmp.command(cmd)
    for cmd, message in REFUSED:
        with pytest.raises(LammpsError, match=message):
            lmp.command(cmd)
        assert not lmp.has_id("compute", cmd.split()[1])
    assert lmp.has_style("compute", "pair/local") and lmp.has_style("compute", "property/local")
    assert lmp.available_styles("compute") == ["pair/local", "property/local"]
    ids = lmp.available_ids("compute")
    assert all(cmd.split()[1] in ids for cmd in ACCEPTED)
    # dump local takes their columns; the column index is checked against the compute's values
    lmp.command("dump 1 all local 10 %s index c_p1[1] c_p1[2] c_d2[1] c_d2[6]" % (tmp_path / "pairs.dump"))
    lmp.command("dump 2 all local 10 %s c_n1[4] c_d1[1]" % (tmp_path / "mixed.dump"))      # (row counts are compared when it is written)
    with pytest.raises(LammpsError, match="out-of-range"):
        lmp.command("dump 3 all local 10 x.dump c_d2[7]")
    with pytest.raises(LammpsError, match="out-of-range"):
        lmp.command("dump 3 all local 10 x.dump c_d1[2]")
    lmp.command("undump 1")
    lmp.command("undump 2")
    with pytest.raises(LammpsError, match="Cannot delete group currently used by a compute"):
        lmp.command("group odd delete")
    lmp.command("uncompute d4")
    assert not lmp.has_id("compute", "d4")
    lmp.close()


@pytest.mark.parametrize("compute, message", [
    ("compute c all property/local natom1 natom2", "No pair style is defined for compute property/local"),
    ("compute c all property/local patom1", "No pair style is defined for compute property/local"),
    ("compute c all pair/local dist eng", "No pair style is defined for compute pair/local"),
])
def test_no_pair_style_at_the_run(tmp_path, compute, message):
    """(a) the checks of the computes' init(): raised by `run` before anything touches a device."""
    head = CHAIN_SCRIPT.replace("pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12\n", "")
    assert "pair_style" not in head
    lmp = _open(tmp_path, head)
    lmp.command(compute)
    with pytest.raises(LammpsError, match=message):
        lmp.command("run 0")
    lmp.close()


def test_extra_fields_are_refused_at_the_run(tmp_path):
    lmp = _open(tmp_path)
    lmp.command("compute x1 all pair/local dist p1")
    with pytest.raises(LammpsError, match="Pair style does not have extra field requested by compute pair/local"):
        lmp.command("run 0")
    lmp.close()


@pytest.mark.parametrize("compute", ["property/local natom1 natom2", "property/local patom1", "pair/local dist eng"])
def test_extract_before_any_run_sets_the_error(tmp_path, compute):
    """(b) no list exists yet: the call sets the error and answers NULL; the bond attributes keep answering from the host."""
    lmp = _open(tmp_path)
    lmp.command("compute c all " + compute)
    lmp.command("compute b all property/local btype batom1 batom2")
    for what in (LMP_SIZE_ROWS, LMP_TYPE_VECTOR):
        with pytest.raises(LammpsError, match="Compute used in dump between runs is not current"):
            lmp.extract_compute("c", LMP_STYLE_LOCAL, what)
    with pytest.raises(LammpsError, match="Compute used in dump between runs is not current"):
        lmp.pair_rows("c")
    assert lmp.extract_compute("b", LMP_STYLE_LOCAL, LMP_SIZE_ROWS) == 499
    assert lmp.pair_rows("b").shape == (499, 3)
    lmp.close()


@pytest.mark.parametrize("name", PR.TABLE_INPUTS)
def test_neigh_rows_are_as_many_as_the_oracles_half_list(name):
    """(c) at `run 0`: the reference program's half list holds every unordered pair once - its count is the yardstick."""
    x = PR.oracle_state(name, 0)[0]
    rows = PR.reference_rows(name, x, "neigh")
    o = run_oracle(PR.run0_script(name, oracle=True), PR.get(name)["system"])
    assert np.array_equal(o.x(), x)
    print("%s: %d NEIGH rows" % (name, len(rows.ids)))
    assert len(rows.ids) == o.neigh_pairs()
    assert len(rows.ids) > 5 * len(x)
    assert np.all(rows.ids[:, 0] < rows.ids[:, 1])
    assert np.array_equal(np.lexsort((rows.ids[:, 1], rows.ids[:, 0])), np.arange(len(rows.ids)))


@pytest.mark.parametrize("name, kind, skin, steps", PR.states())
def test_state_has_no_undecided_pair(name, kind, skin, steps):
    """(d) the allowed number of undecided pairs is zero, at `run 0` and at the oracle's positions after the steps; a run of
    steps ends without a rebuild at its last step (the list the rows come from is older than the positions)."""
    x, builds, bonds = PR.oracle_state(name, steps)
    rows = PR.reference_rows(name, x, kind, skin, bonds=bonds)
    print("%s %s after %d steps: %d rows, %d builds" % (name, kind, steps, len(rows.ids), builds))
    assert rows.undecided == []
    assert len(rows.ids) > 0
    if steps:
        assert builds == PR.oracle_state(name, steps - 1)[1]
        assert np.abs(x - PR.oracle_state(name, 0)[0]).max() > 1e-3
    if name == "le_small":
        # the firing created extruder bonds between beads inside the pair cutoff: their pairs have left the rows
        new = [tuple(b[1:]) for b in bonds.tolist() if b[0] == 2]
        before = PR.reference_rows(name, x, kind, skin)          # (the same positions under the data file's bonds)
        had = set(map(tuple, before.ids[:, :2].tolist()))
        has = set(map(tuple, rows.ids[:, :2].tolist()))
        print("new extruder bonds %d, of them inside the cutoff now %d" % (len(new), sum(1 for b in new if b in had)))
        assert len(new) >= 3 and sum(1 for b in new if b in had) >= 3 and not any(b in has for b in new)


def test_reference_rows_follow_the_special_weights():
    """hubs-harmonic under `special_bonds lj 0 0.3 0.7`: no 1-2 pair is a row, 1-3 and 1-4 pairs are, with their factor; the
    bead without a neighbor has no row; a group keeps the rows with both members."""
    inp = PR.get("hubs-harmonic")
    s = inp["system"]
    x = PR.oracle_state("hubs-harmonic", 0)[0]
    rows = PR.reference_rows("hubs-harmonic", x, "pair")
    sp = PR.levels_of(len(x), s["bonds"])
    level_of = lambda r: np.array([sp.get(a, {}).get(b, 0) for a, b in r.ids[:, :2].tolist()])
    neigh = PR.reference_rows("hubs-harmonic", x, "neigh")
    levels, nlevels = level_of(rows), level_of(neigh)
    print("levels of the PAIR rows", np.bincount(levels, minlength=4), "of the NEIGH rows", np.bincount(nlevels, minlength=4))
    assert (levels != 1).all() and (nlevels != 1).all()
    assert (levels == 2).sum() > 0 and (levels == 3).sum() > 0 and (nlevels == 2).sum() > 20 and (nlevels == 3).sum() > 20
    from force_inputs import INPUTS
    lone = INPUTS["hubs-harmonic"]()["lone"]
    assert lone not in rows.ids[:, :2]
    assert lone not in neigh.ids[:, :2]
    odd = (np.arange(1, len(x) + 1) % 2) == 1
    sub = PR.reference_rows("hubs-harmonic", x, "pair", member=odd)
    both = (rows.ids[:, 0] % 2 == 1) & (rows.ids[:, 1] % 2 == 1)
    assert np.array_equal(sub.ids, rows.ids[both]) and np.array_equal(sub.vals, rows.vals[both]) and 0 < both.sum() < len(both)
    # the energy column sums to the pair energy of the long-double force reference
    import force_compare as FC
    assert FC.relerr(rows.vals[:, 1].sum(), FC.reference_run0("hubs-harmonic").evdwl) < 1e-15


def test_nudged_state_has_no_undecided_pair():
    """(d) the state test_subset_scatter_changes_the_pair_rows compares after its scatter: one bead of `tiny` moved 0.15 away
    from its farthest PAIR partner - that row leaves, nothing is undecided, and the list of the run-0 build (skin 0.4) still holds
    every pair inside its cutoff (no bead moved more than half the skin)."""
    x = PR.oracle_state("tiny", 0)[0]
    before = PR.reference_rows("tiny", x, "pair")
    a, b, pos = PR.nudge("tiny", x)
    assert np.abs(np.linalg.norm(pos - x[a - 1]) - 0.15) < 1e-12 and 0.15 < 0.5 * 0.4
    x1 = x.copy()
    x1[a - 1] = pos
    after = PR.reference_rows("tiny", x1, "pair")
    assert after.undecided == [] and before.undecided == []
    assert [a, b] in before.ids[:, :2].tolist() and [a, b] not in after.ids[:, :2].tolist() and len(after.ids) < len(before.ids)
    listed = set(map(tuple, PR.reference_rows("tiny", x, "neigh").ids[:, :2].tolist()))
    assert all(tuple(r) in listed for r in after.ids[:, :2].tolist())
