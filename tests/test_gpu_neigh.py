"""The device neighbor list, entry by entry, against brute force (neigh_reference.py).

Every case runs a script on the engine, fetches the list of the last build through the test hook
lammps_le_test_neighbor_list (tags, decoded special bits, the positions the list was built from) and asserts
 (a) after a `run 0`, that those positions are the current ones, bit for bit (and the wrapped input's);
 (b) that the pair entries are exactly the reference's: no duplicate, none missing, none too many, every special code
     right, (i, j) wherever (j, i) is - computed in long double from the positions of (a), none of whose pairs is
     UNDECIDED (asserted here on those positions, and for every input without a GPU in test_neigh_reference_cpu.py);
 (c) that the bond entries that open each bead's list are the bonds the bead stores, as a multiset of (type, partner) -
     both ends of a bond carry it (k_bond_table reads the per-atom bond tables, which hold every bond on both atoms);
 (d) that stat("neigh_pairs") counts the entries the hook returned;
 (e) where the case is about the path a rebuild takes, that stat("rebuild_plan") - the plan the last rebuild executed - is
     what the test hook lammps_le_test_rebuild_plan answers for the facts the case is meant to produce (rebuild_rules.py).

Out of scope: runs whose special lists have become asymmetric (k_build_neigh_asym: the expected code there depends on the
reference's half-list storage order; covered through forces by the LE fuzz suites), and angles."""
import collections
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import neigh_inputs as I
import neigh_reference as R
import rebuild_rules as P
from neigh_worker import fetch_list
from systems import CHAIN_SCRIPT, run_oracle, run_product, wrap_into_box

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C = I.CUTNEIGH
FENE = ((0.0, 1.0, 1.0), (0.0, 1.0, 1.0))


def check_list(L, system, topo, neigh_pairs, weights=FENE, x_now=None, bonds=None, cutneigh=C):
    """(b), (c), (d) and - with x_now, the engine's current positions - (a).  L: fetch_list() (one rank) or the ranks' lists
    joined; topo = (num_bond, bond_type, bond_atom) gathered from the same handle.  bonds: the bonds the tables have to hold,
    rows (type, a, b) - the data file's unless a fix has edited them (test_gpu_le_state.py); the special codes always follow
    the search over the stored bonds.  cutneigh: the list cutoff, if not the chain scripts'.  Returns (x by tag, reference)."""
    n = len(system["x"])
    box = np.asarray(system["box"], dtype=np.float64)
    owned = np.asarray(L["owned"])
    assert len(owned) == n and np.array_equal(np.sort(owned), np.arange(1, n + 1)), "every bead is owned exactly once"
    x = np.empty((n, 3))
    x[owned - 1] = L["xbuild"]
    if x_now is not None:
        assert np.array_equal(x, x_now), "list was not built from the current positions"
        assert np.array_equal(x, wrap_into_box(system)[0])
    assert (x >= box[:, 0]).all() and (x < box[:, 1]).all()
    ref = R.reference_pairs(x, box, cutneigh)
    assert R.undecided(ref) == []
    num_bond, bond_type, bond_atom = (np.asarray(t).reshape(n, -1) for t in topo)
    stored = collections.Counter()
    graph = []
    for i in np.nonzero(num_bond[:, 0])[0]:
        for m in range(num_bond[i, 0]):
            stored[(int(i) + 1, int(bond_type[i, m]), int(bond_atom[i, m]))] += 1
            graph.append((int(bond_type[i, m]), int(i) + 1, int(bond_atom[i, m])))
    held = np.asarray(system["bonds"] if bonds is None else bonds).reshape(-1, 3)
    for t, a, b in held.tolist():          # both ends carry the bond
        assert stored[(a, t, b)] == 1 and stored[(b, t, a)] == 1
    assert sum(stored.values()) == 2 * len(held)
    listed_bonds = collections.Counter(zip(L["btag"].tolist(), L["btype"].tolist(), L["bjtag"].tolist()))
    assert listed_bonds == stored, "bond entries differ from the stored bonds"
    expected = R.expected_entries(ref, np.arange(1, n + 1), n, graph, *weights)
    x_by_tag = np.vstack([np.zeros((1, 3)), x])
    rep = R.compare((L["itag"], L["jtag"], L["code"]), expected, (x_by_tag, box, cutneigh))
    print("pair entries %d, expected %d, %s" % (len(L["itag"]), len(expected), rep.counts()))
    assert rep.ok, str(rep)
    assert neigh_pairs == len(L["itag"])
    return x, ref


def planned(topo, n, weights=FENE, minimg=1, **facts):
    """(e): the hook's plan for a run of the chain scripts on `topo` (the gathered bond tables of n beads: their width is the
    bonds per atom) under special weights `weights`; `facts` name what differs from the setup build of a handle's first run
    on one GPU (bond records to pack, nothing binned, no physical records yet)."""
    bpa = np.asarray(topo[1]).size // n
    lj, coul = weights
    sf = [0 if (a, b) == (0.0, 0.0) else 1 if a == 1.0 else 2 for a, b in zip(lj, coul)]          # Engine::special_flag
    f = dict(bonds_dirty=1, bond_minimg=int(minimg), bpa=bpa, bond_pack_stride=(1 + bpa + 3) & ~3, sf1=sf[0], sf2=sf[1], sf3=sf[2])
    f.update(facts)
    bits, _, known = P.hook()(P.facts(**f))
    assert known == 1 and bits == P.expected(P.facts(**f), {k: os.environ[k] for k in P.SWITCHES if k in os.environ})[0]
    return bits


def last_rebuild(script, system, builds, steps):
    """Facts of the last rebuild inside a run of `steps` steps that rebuilt `builds` times: the packed records are current,
    and the check is deferred behind the next step kernel unless the rebuild fell on the run's last step, which is a thermo
    step (the oracle tells: one step fewer, one build fewer)."""
    on_last_step = run_oracle(script.replace("run %d" % steps, "run %d" % (steps - 1)), system).neigh_builds() != builds
    return dict(bonds_dirty=0, can_defer=int(not on_last_step), builds=int(builds) - 1)


def run_and_check(system, script, tmp_path, weights=FENE, current=True):
    lmp = run_product(script, system, tmp_path)
    L = fetch_list(lmp)
    topo = (lmp.gather("num_bond"), lmp.gather("bond_type"), lmp.gather("bond_atom"))
    x, ref = check_list(L, system, topo, lmp.stat("neigh_pairs"), weights, lmp.gather("x") if current else None)
    return lmp, L, x, ref


def run_in_children(world, system, script, tmp_path, env=None):
    """The script in `world` processes of their own (neigh_worker.py); returns the ranks' outputs."""
    session = uuid.uuid4().hex[:12]
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "neigh_worker.py"), str(r), str(world), session, sysfile,
                               scriptfile, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              env=dict(os.environ, **(env or {}))) for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [dict(np.load("%s.r%d.npz" % (out, r))) for r in range(world)]


def joined(ranks):
    return {k: np.concatenate([r[k] for r in ranks]) for k in ("itag", "jtag", "code", "btag", "bjtag", "btype", "owned", "xbuild")}


# ---- 1, 2: the chain; other origins; a box with three different cell counts; z-major rows -------------------------------
@pytest.mark.parametrize("origin", [0, 1, 2])
def test_chain_at_origin(tmp_path, origin):
    run_and_check(I.chain_at(origin), CHAIN_SCRIPT + "run 0\n", tmp_path)


def test_noncubic_box_partial_row_tiles(tmp_path):
    s = I.noncubic_chain(1)
    ncx, ncy, ncz = I.cell_counts(s["box"])
    assert len({ncx, ncy, ncz}) == 3 and ncy > 16 and ncz > 16 and ncy % 16 and ncz % 16
    run_and_check(s, CHAIN_SCRIPT + "run 0\n", tmp_path)


def test_noncubic_box_without_row_tiles(tmp_path):
    """LAMMPS_LE_NO_ROW_TILES is latched when the device state is allocated: a process of its own."""
    s = I.noncubic_chain(1)
    (r,) = run_in_children(1, s, CHAIN_SCRIPT + "run 0\n", tmp_path, env={"LAMMPS_LE_NO_ROW_TILES": "1"})
    check_list(r, s, (r["num_bond"], r["bond_type"], r["bond_atom"]), r["neigh_pairs"][0], FENE, r["x"])


# ---- 3, 7: the cutoff ladder, and the same list from the FP64-only build -----------------------------------------------
@pytest.mark.parametrize("origin", [0, 1, 2])
def test_cutoff_ladder(tmp_path, origin, monkeypatch):
    s, meta = I.ladder(origin)
    assert len(meta) >= 300
    lmp, L, x, ref = run_and_check(s, I.ZERO_SCRIPT + "run 0\n", tmp_path)
    nchain = len(I.chain_at(origin)["x"])
    listed = set(zip(L["itag"].tolist(), L["jtag"].tolist()))
    for m in meta:          # (implied by the comparison; spelled out for the probes)
        a = nchain + m["row"] + 1
        assert ((a, a + 1) in listed) == (m["side"] < 0) and ((a + 1, a) in listed) == (m["side"] < 0), m
    lmp.close()
    monkeypatch.setenv("LAMMPS_LE_BUILD_FP64", "1")          # read at every run command
    lmp64 = run_product(I.ZERO_SCRIPT + "run 0\n", s, tmp_path)
    L64 = fetch_list(lmp64)
    for k in ("owned", "itag", "jtag", "code", "btag", "bjtag", "btype"):
        assert np.array_equal(L[k], L64[k]), "the FP32-prefiltered build and the FP64 build differ in " + k
    assert np.array_equal(L["xbuild"], L64["xbuild"])
    lmp64.close()


# ---- 4: a dense cluster: rows too long to stage, a table too short ------------------------------------------------------
def test_dense_cluster_regrows_the_table(tmp_path):
    s = I.dense_cluster()
    lmp, L, x, ref = run_and_check(s, I.ZERO_SCRIPT + "run 0\n", tmp_path)
    n = len(s["x"])
    assert lmp.stat("maxneigh") > I.initial_maxneigh(n, s["box"])
    per_bead = np.bincount(L["itag"], minlength=n + 1)
    assert (per_bead[n + 1 - I.CLUSTER_BEADS:] >= I.CLUSTER_BEADS - 1).all() and per_bead.max() <= lmp.stat("maxneigh")
    # (e) the last plan executed is the regrow pass: the bond table and the build, nothing else
    topo = (lmp.gather("num_bond"), lmp.gather("bond_type"), lmp.gather("bond_atom"))
    plan = int(lmp.stat("rebuild_plan"))
    assert plan == planned(topo, n, FENE, lmp.stat("bond_minimg"), regrow=1, bonds_dirty=0, phys_valid=1)
    assert plan & P.LAUNCHES == P.BOND_TABLE | P.BUILD
    lmp.close()


# ---- 5: beads on faces and on cell boundaries ---------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [0, 1])
def test_faces_and_cell_boundaries(tmp_path, origin):
    s = I.faces(origin)
    box = np.asarray(s["box"])
    outside = ((s["x"] < box[:, 0]) | (s["x"] >= box[:, 1])).any(axis=1).sum()
    assert outside >= 12          # beads that have to wrap
    run_and_check(s, I.ZERO_SCRIPT + "run 0\n", tmp_path)


# ---- 6: special neighbors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(I.SPECIAL_CASES))
def test_special_codes(tmp_path, case):
    args, lj, coul, hub = I.SPECIAL_CASES[case]
    s = I.special_chain(hub)
    lmp, L, x, ref = run_and_check(s, CHAIN_SCRIPT.replace("special_bonds fene", "special_bonds " + args) + "run 0\n", tmp_path, (lj, coul))
    codes = np.bincount(L["code"], minlength=4)
    print("codes", codes)
    if case == "lj-fractional":
        assert codes[2] > 100 and codes[3] > 100 and codes[1] == 0
    elif case == "lj-0-1-1-coul-1-1-1":
        assert codes[1] > 1000 and codes[2] == 0 and codes[3] == 0
    else:
        assert codes[1] == codes[2] == codes[3] == 0
    # (e) where the exclusions come from and which build stores them: as the weights and the bonds per atom say
    topo = (lmp.gather("num_bond"), lmp.gather("bond_type"), lmp.gather("bond_atom"))
    plan = int(lmp.stat("rebuild_plan"))
    assert plan == planned(topo, len(x), (lj, coul), lmp.stat("bond_minimg"))
    bpa = np.asarray(topo[1]).size // len(x)
    assert bool(plan & P.EXCL_BPART) == (args == "fene" and bpa <= 4) and (bpa <= 4) == (not hub)
    assert bool(plan & P.NOSP) == (case == "lj-1-1-1") and not plan & P.ASYM
    assert bool(plan & P.FRAC) == (case in ("lj-fractional", "lj-0-1-1-coul-1-1-1"))
    lmp.close()


# ---- 3b: wavefronts that skip the minimum image, and wavefronts that must not ----------------------------------------------
def test_interior_and_almost_interior_wavefronts(tmp_path):
    """Every wavefront of this build is one x zone of one row of cells (neigh_inputs.aligned_rows): one of them is wholly
    interior and skips the minimum image; two lie between cutneigh / 2 and cutneigh from a face and have neighbors across it."""
    s = I.aligned_rows()
    lmp, L, x, ref = run_and_check(s, I.ZERO_SCRIPT + "run 0\n", tmp_path)
    assert lmp.stat("maxneigh") > I.initial_maxneigh(len(x), s["box"])
    lmp.close()


# ---- 8: rebuilds inside a run --------------------------------------------------------------------------------------------
# the step kernel picks its shape by system size, from switches read at every run command: small systems (these) run four lanes
# per bead with loads issued ahead; the shape of the large ones tests the displacement against the FLOAT copy of the build
# positions inside `hold_band` and bins the new positions itself, so that the next rebuild skips k_wrap_bin
SHAPES = {"small-system-shape": {}, "throughput-shape": {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}}
# the chain has no bond of type 2: with that type's R0 at 1.5 instead of 4.0 every 2 R0 is below half the 6.3-wide box of
# rebuild_chain, the per-step minimum image is provably the frozen one (stat "bond_minimg" 1) and the permute pass writes
# the bond-partner table - the path of the benchmark systems
MINIMG_SCRIPT = CHAIN_SCRIPT.replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 30.0 1.5 1.0 1.0")
assert MINIMG_SCRIPT != CHAIN_SCRIPT


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rebuilds_inside_a_run(tmp_path, shape):
    """Offset non-cubic box, 60 steps of Langevin dynamics: the list of the LAST build (in the throughput shape: fed by the
    bins the step kernel wrote) against the positions it was built from; the number of builds and the trajectory against
    the oracle.  Position bound: the project's 1e-9 for 100 steps in the 16.9-wide box of test_nve_trajectory, scaled by the
    coordinate magnitude M / 16.9 (every rounding seed scales with the ulp of a coordinate, the chaotic growth does not).
    Measured on an MI355X, both shapes: 7 builds, max |x - x_oracle| 2.7e-12 (bound 2.4e-7)."""
    s = I.rebuild_chain()
    script = MINIMG_SCRIPT + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nrun 60\n"
    (r,) = run_in_children(1, s, script, tmp_path, env=SHAPES[shape])
    x, ref = check_list(r, s, (r["num_bond"], r["bond_type"], r["bond_atom"]), r["neigh_pairs"][0])
    builds = r["builds"][0]
    assert builds >= 3
    o = run_oracle(script, s)
    assert builds == o.neigh_builds()
    # (e) the last rebuild: fed by the step kernel's bins in the throughput shape, by k_wrap_bin in the other; the permute
    # writes the bond table from the physical records either way
    binned = int(shape == "throughput-shape")
    plan = int(r["rebuild_plan"][-1])
    assert r["bond_minimg"][0] == 1
    assert plan == planned((r["num_bond"], r["bond_type"], r["bond_atom"]), len(x), bins_ready=binned, counts_dirty=binned, phys_valid=1,
                           **last_rebuild(script, s, builds, 60))
    assert bool(plan & P.PREBINNED) == binned and bool(plan & P.WRAP_BIN) == (not binned)
    assert plan & P.PERMUTE_BONDS and plan & P.PERMUTE_PHYS and not plan & (P.BOND_TABLE | P.BOND_PACK_PHYS)
    box = np.asarray(s["box"])
    prd = box[:, 1] - box[:, 0]
    dev = np.abs((r["x"] + r["image"] * prd) - (o.x() + o.image() * prd)).max()
    M = np.abs(box).max()
    print("neigh_builds %d, max |x - x_oracle| %.3e (bound %.3e)" % (builds, dev, 1e-9 * max(1.0, M / 16.9)))
    assert dev <= 1e-9 * max(1.0, M / 16.9)
    assert np.abs(r["x"] - x).max() > 1e-3          # (the list is the last build's, not the current positions')


# ---- 8a: the bond table by its other paths --------------------------------------------------------------------------------
# frozen images (a bond style that is not fene; fene with LAMMPS_LE_FREEZE_IMAGES=1): k_bond_table writes the table and the
# image words, the permute moves beads only.  A hub of six bonds: records of two int4, the permute writes the table from the
# records by tag (bond type 2 with R0 3.5: 2 R0 stays below half the 15.8-wide box, the minimum image holds).
HARMONIC = CHAIN_SCRIPT.replace("bond_style fene", "bond_style harmonic").replace("bond_coeff 1 30.0 1.5 1.0 1.0", "bond_coeff 1 30.0 1.05") \
    .replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 30.0 1.05")
BOND_PATHS = {"harmonic": (HARMONIC, {}), "fene-frozen": (MINIMG_SCRIPT, {"LAMMPS_LE_FREEZE_IMAGES": "1"}),
              "fene-hub": (CHAIN_SCRIPT.replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 5.0 3.5 1.0 1.0"), {})}
assert "bond_style harmonic" in HARMONIC and HARMONIC.count("1.05") == 2 and "3.5 1.0 1.0" in BOND_PATHS["fene-hub"][0]


@pytest.mark.parametrize("steps", [0, 60])
@pytest.mark.parametrize("case", sorted(BOND_PATHS))
def test_bond_table_paths(tmp_path, monkeypatch, case, steps):
    """The setup build (`run 0`) and the last rebuild inside a run of 60 steps (in the throughput shape of the step kernel,
    which bins for the rebuild): the list entry by entry, the number of builds against the oracle's, and the plan."""
    head, env = BOND_PATHS[case]
    for k, v in dict(env, **(SHAPES["throughput-shape"] if steps else {})).items():
        monkeypatch.setenv(k, v)
    s = I.special_chain(True) if case == "fene-hub" else I.rebuild_chain()
    script = head + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 904297\nrun %d\n" % steps
    lmp, L, x, ref = run_and_check(s, script, tmp_path, current=steps == 0)
    builds = lmp.stat("neigh_builds")
    o = run_oracle(script, s)
    assert builds == o.neigh_builds() and (steps == 0 or builds >= 3)
    topo = (lmp.gather("num_bond"), lmp.gather("bond_type"), lmp.gather("bond_atom"))
    bpa, minimg = np.asarray(topo[1]).size // len(x), lmp.stat("bond_minimg")
    plan = int(lmp.stat("rebuild_plan"))
    moved = case == "fene-hub"          # the permute writes the table
    assert minimg == int(moved) and bpa == (6 if moved else 3)
    later = dict(last_rebuild(script, s, builds, steps), phys_valid=0, bins_ready=1, counts_dirty=1) if steps else {}
    assert plan == planned(topo, len(x), FENE, minimg, **later)
    assert bool(plan & P.PERMUTE_BONDS) == moved and bool(plan & P.BOND_TABLE) == (not moved) and bool(plan & P.FROZEN_IMAGES) == (not moved)
    assert not plan & (P.PERMUTE_PHYS | P.BOND_PACK_PHYS) and bool(plan & P.PREBINNED) == (steps > 0) and bool(plan & P.WRAP_BIN) == (steps == 0)
    if case == "fene-frozen":          # the same plan as for bonds that cannot do without frozen images
        monkeypatch.delenv("LAMMPS_LE_FREEZE_IMAGES")
        assert plan == planned(topo, len(x), FENE, 0, **later)
    lmp.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("sign", [+1, -1])
def test_rebuild_trigger_at_the_edge_of_its_band(tmp_path, sign, shape):
    """One free bead whose displacement misses skin/2 by 5e-5 at the tenth step while the float copy of its start is off by
    1e-4 the other way (neigh_inputs.trigger_probe): the rebuild has to come when the FP64 test says so."""
    s = I.trigger_probe(sign)
    script = I.EPS0_SCRIPT + "fix 1 all nve\nrun %d\n" % I.TRIGGER_STEPS
    (r,) = run_in_children(1, s, script, tmp_path, env=SHAPES[shape])
    check_list(r, s, (r["num_bond"], r["bond_type"], r["bond_atom"]), r["neigh_pairs"][0])
    o = run_oracle(script, s)
    assert o.neigh_builds() == I.TRIGGER_BUILDS[sign]
    assert r["builds"][0] == o.neigh_builds()


# ---- 9: z slabs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_decomposed(tmp_path, world):
    """Every rank hands out the lists of the beads it owns, ghost neighbors by their tag: the union is the full list."""
    s, meta = I.slab_ladder()
    ranks = run_in_children(world, s, I.ZERO_SCRIPT + "run 0\nrun 0\n", tmp_path)
    assert all(len(r["owned"]) > 0 for r in ranks)
    r0 = ranks[0]
    # (e) both setup builds on every rank: map[] filled before the first only, nothing prebinned, the decomposed build, the
    # send lists reordered for direct receive
    topo = (r0["num_bond"], r0["bond_type"], r0["bond_atom"])
    dd = dict(decomposed=1, row_tile=0, bond_minimg=r0["bond_minimg"][0])
    first, second = planned(topo, len(s["x"]), map_stale=1, **dd), planned(topo, len(s["x"]), **dd)
    assert first == second | P.MAP_FILL and not second & (P.MAP_FILL | P.PREBINNED | P.WRAP_BIN | P.PERMUTE_BONDS)
    assert (second & P.DDCODE) >> P.DDCODE_SHIFT == 1 and second & P.DIRECT_RECV and second & P.BOND_TABLE
    assert all(r["rebuild_plan"].tolist() == [first, second] for r in ranks)
    assert sum(len(r["itag"]) for r in ranks) == r0["neigh_pairs"][0]
    check_list(joined(ranks), s, (r0["num_bond"], r0["bond_type"], r0["bond_atom"]), r0["neigh_pairs"][0], FENE, r0["x"])
    # the probes really straddle this run's slab boundaries: some pair has its two beads on different ranks
    owner = {}
    for k, r in enumerate(ranks):
        owner.update((int(t), k) for t in r["owned"])
    nchain = len(s["x"]) - 2 * len(meta)
    split = sum(1 for m in meta if owner[nchain + m["row"] + 1] != owner[nchain + m["row"] + 2])
    assert split >= 40
