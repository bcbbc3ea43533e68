"""CPU tests of the neighbor-list reference (neigh_reference.py) and of the inputs of test_gpu_neigh.py (neigh_inputs.py).

They pin the brute-force reference to the CPU oracle, and they prove - without a GPU - the two properties the GPU tests
lean on: no input holds an UNDECIDED pair (so the list comparison leaves nothing out), and the cutoff ladder has members
on both sides of the cutoff inside and outside the FP32 error band of the list build."""
import functools
import os

import numpy as np
import pytest

import neigh_inputs as I
import neigh_reference as R
from systems import CHAIN_SCRIPT, lattice_chain, run_oracle, wrap_into_box

C = I.CUTNEIGH
FENE = ((0.0, 1.0, 1.0), (0.0, 1.0, 1.0))


@functools.lru_cache(maxsize=None)
def reference_of(name):
    s = INPUTS[name]()
    x, _ = wrap_into_box(s)          # what read_data makes of the coordinates
    return s, x, R.reference_pairs(x, s["box"], C)


INPUTS = {
    "chain-origin0": lambda: I.chain_at(0), "chain-origin1": lambda: I.chain_at(1), "chain-origin2": lambda: I.chain_at(2),
    "noncubic": lambda: I.noncubic_chain(1),
    "ladder-origin0": lambda: I.ladder(0)[0], "ladder-origin1": lambda: I.ladder(1)[0], "ladder-origin2": lambda: I.ladder(2)[0],
    "dense-cluster": lambda: I.dense_cluster(),
    "faces-origin0": lambda: I.faces(0), "faces-origin1": lambda: I.faces(1),
    "special-chain": lambda: I.special_chain(False), "special-hub": lambda: I.special_chain(True),
    "aligned-rows": lambda: I.aligned_rows(), "trigger-probe": lambda: I.trigger_probe(1),
    "rebuild-start": lambda: I.rebuild_chain(), "slab-ladder": lambda: I.slab_ladder()[0],
}


def half_count(entries):
    assert all((b, a) in entries for a, b in entries)
    return len(entries) // 2


def test_reference_pair_count_equals_the_oracle():
    s = lattice_chain(4096, jitter=0.08)
    o = run_oracle(CHAIN_SCRIPT + "run 0\n", s)
    ref = R.reference_pairs(s["x"], s["box"], C)
    assert R.undecided(ref) == []
    n = len(s["x"])
    entries = R.expected_entries(ref, np.arange(1, n + 1), n, s["bonds"], *FENE)
    assert half_count(entries) == o.neigh_pairs()
    assert len(ref.i) // 2 - len(s["bonds"]) == o.neigh_pairs()       # (every bond of this chain is shorter than the cutoff)


def star_molecule():
    """A centre bonded to six arms of two beads each, in a box of its own."""
    pts, bonds = [(4.0, 4.0, 4.0)], []
    for d in range(3):
        for sgn in (-1.0, 1.0):
            for k in (1, 2):
                p = [4.0, 4.0, 4.0]
                p[d] += sgn * k
                pts.append(tuple(p))
                bonds.append((2, 1 if k == 1 else len(pts) - 1, len(pts)))
    n = len(pts)
    return dict(box=np.array([[0.0, 8.0]] * 3), x=np.array(pts), v=np.zeros((n, 3)), type=np.ones(n, dtype=np.int32),
                mol=np.ones(n, dtype=np.int32), image=np.zeros((n, 3), dtype=np.int32), bonds=np.array(bonds, dtype=np.int32),
                ntypes=1, nbondtypes=2, mass=[1.0], extra_bond=0, extra_special=0, atom_style="bond")


@pytest.mark.parametrize("which", ["chain-with-i-i+2-bonds", "star"])
def test_reference_specials_equal_the_oracle(which):
    s = I.special_chain(False) if which.startswith("chain") else star_molecule()
    o = run_oracle(CHAIN_SCRIPT.replace("special_bonds fene", "special_bonds lj 0.0 0.0 0.0") + "run 0\n", s)
    ns, sp = o.special_table()
    n = len(s["x"])
    mine = R.reference_specials(n, s["bonds"])
    levels_seen = set()
    for t in range(1, n + 1):
        theirs = {}
        for k in range(ns[t - 1, 2]):
            theirs[int(sp[t - 1, k])] = 1 if k < ns[t - 1, 0] else 2 if k < ns[t - 1, 1] else 3
        assert theirs == mine.get(t, {}), t
        levels_seen.update(theirs.values())
    assert levels_seen == {1, 2, 3}


def test_expected_code_restates_special_flag():
    lj, coul = (0.0, 0.3, 1.0), (0.0, 0.0, 0.5)
    assert R.expected_code(0, lj, coul) == 0
    assert R.expected_code(1, lj, coul) is None           # both weights 0: the pair is not listed
    assert R.expected_code(2, lj, coul) == 2              # fractional weight: listed with its level
    assert R.expected_code(3, lj, coul) == 0              # lj weight 1: an ordinary entry, whatever coul says
    assert R.expected_code(1, (0.0, 1.0, 1.0), (1.0, 1.0, 1.0)) == 1      # kept for its coul weight, with the level bits


def test_compare_names_every_kind_of_error():
    """One entry dropped and another one stored twice leaves the sum the suite used to check unchanged."""
    s = lattice_chain(512)
    n = len(s["x"])
    ref = R.reference_pairs(s["x"], s["box"], C)
    exp = R.expected_entries(ref, np.arange(1, n + 1), n, s["bonds"], *FENE)
    keys = sorted(exp)
    arr = lambda ks, codes: (np.array([k[0] for k in ks]), np.array([k[1] for k in ks]), np.array(codes))
    assert R.compare(arr(keys, [0] * len(keys)), exp).ok
    bad = keys[1:] + [keys[5]]                       # same length: keys[0] missing, keys[5] twice
    rep = R.compare(arr(bad, [0] * len(bad)), exp, (np.vstack([np.zeros(3), s["x"]]), s["box"], C))
    assert rep.counts() == dict(duplicates=1, missing=1, extra=0, wrong_code=0, asymmetric=1)
    assert rep.missing[0][:2] == keys[0] and rep.duplicates[0][:2] == keys[5]
    assert "r2_ld" in str(rep) and "r2_f32" in str(rep) and "band" in str(rep)
    codes = [0] * len(keys)
    codes[7] = 2
    rep = R.compare(arr(keys, codes), exp)
    assert rep.counts() == dict(duplicates=0, missing=0, extra=0, wrong_code=1, asymmetric=2)
    stranger = (keys[0][0], keys[0][0] % n + 300 if (keys[0][0], keys[0][0] % n + 300) not in exp else None)
    assert stranger[1] is not None
    rep = R.compare(arr(keys + [stranger], [0] * (len(keys) + 1)), exp)
    assert rep.counts() == dict(duplicates=0, missing=0, extra=1, wrong_code=0, asymmetric=1)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_input_has_no_undecided_pair(name):
    s, x, ref = reference_of(name)
    box = np.asarray(s["box"])
    assert (x >= box[:, 0]).all() and (x < box[:, 1]).all()
    assert ref.delta == 16.0 * 2.0 ** -53 * C * ((box[:, 1] - box[:, 0]).max() + C)
    assert R.undecided(ref) == []
    assert len(ref.i) > 10 * len(x)           # (a list worth checking: more than 10 neighbors per bead)


@pytest.mark.parametrize("origin", [0, 1, 2])
def test_ladder_straddles_the_fp32_band(origin):
    s, meta = I.ladder(origin)
    _, x, ref = reference_of("ladder-origin%d" % origin)
    box = np.asarray(s["box"])
    # the band of the list build, restated from kernels_neigh.hip rebuild_lists.  If that formula is ever narrowed, the rungs
    # below (BAND_RUNGS are fractions of THIS band) have to be derived again from the new one.
    M = np.abs(box).max()
    e_d = 8.0 * M * 5.97e-8
    band = float(np.float32(4.0 * 1.5 * C * e_d + 3.0 * e_d * e_d + 1e-5 * C * C))
    assert band == R.fp32_band(box, C)
    dl = R.delta(box, C)
    assert len(meta) >= 300
    nchain = len(I.chain_at(origin)["x"])
    c2 = R.LD(C) * R.LD(C)
    listed = set(zip(ref.i.tolist(), ref.j.tolist()))
    for m in meta:                                   # every probe is what its record says, as the reference sees it
        a, b = nchain + m["row"], nchain + m["row"] + 1
        g = R.sep2_ld(x[a], x[b], box) - c2
        assert float(g) == m["gap"] and abs(m["gap"]) > dl and (m["gap"] > 0) == (m["side"] > 0)
        assert ((a, b) in listed) == (m["side"] < 0)
    count = lambda rung, side: sum(1 for m in meta if m["rung"] == rung and m["side"] == side)
    ncombo = len({(m["place"], m["direction"], m["dim"]) for m in meta})
    assert ncombo == 21
    for side in (-1, 1):
        gaps = np.array([abs(m["gap"]) for m in meta if m["side"] == side])
        assert (gaps < band).sum() >= 100 and (gaps > band).sum() >= 40      # inside and outside the band, on this side
        assert gaps.min() < 8 * dl if origin == 0 else gaps.min() < 128 * dl
        for place in ("deep", "face", "nearface", "edge", "corner"):
            assert any(m["place"] == place and m["side"] == side and abs(m["gap"]) < 1e4 * dl for m in meta), place
        for f in I.BAND_RUNGS:
            assert count(("band", f), side) == ncombo
        for mult in I.DELTA_RUNGS:
            inside = all(abs(m["gap"]) < band for m in meta if m["rung"] == ("delta", mult))
            assert inside                                          # every delta rung lies inside the band
            if origin == 0 or mult >= 1e3:                         # (at |x| ~ 4000 a coordinate's ulp, 4.5e-13, is wider than
                assert count(("delta", mult), side) == ncombo      #  the finest rungs: some of their probes cannot be realised)
            elif mult >= 64:
                assert count(("delta", mult), side) >= ncombo - 3
            else:
                assert count(("delta", mult), side) >= 6


def test_noncubic_box_has_three_different_cell_counts():
    for s in (I.noncubic_chain(1), I.rebuild_chain()):
        ncx, ncy, ncz = I.cell_counts(s["box"])
        assert (ncx, ncy, ncz) == I.NONCUBIC_CELLS
        assert len({ncx, ncy, ncz}) == 3 and ncy > 16 and ncz > 16 and ncy % 16 and ncz % 16
    box = np.asarray(I.slab_ladder()[0]["box"])
    assert box[2, 1] - box[2, 0] >= 30.0 and I.cell_counts(box)[:2] == I.NONCUBIC_CELLS[:2]


def test_dense_cluster_overflows_stage_and_table():
    s, x, ref = reference_of("dense-cluster")
    box = np.asarray(s["box"])
    nc = I.cell_counts(box)
    cell = np.minimum(((x - box[:, 0]) * (np.array(nc) / (box[:, 1] - box[:, 0]))).astype(int), np.array(nc) - 1)
    cl = cell[-I.CLUSTER_BEADS:]
    assert (cl[:, 1] == cl[0, 1]).all() and (cl[:, 2] == cl[0, 2]).all()          # one (y, z) row of cells
    row = cell[(cell[:, 1] == cl[0, 1]) & (cell[:, 2] == cl[0, 2])]
    cx = int(np.median(cl[:, 0]))
    window = ((row[:, 0] >= cx - 4) & (row[:, 0] <= cx + 4)).sum()
    assert window > 128               # a wavefront's row interval cannot be staged (STAGE_CAP slots) ...
    longest = np.bincount(ref.i, minlength=len(x)).max()
    assert longest >= I.CLUSTER_BEADS - 1 > I.initial_maxneigh(len(x), box)      # ... and the first table is too short


def test_special_systems_reach_every_branch():
    for hub in (False, True):
        s = I.special_chain(hub)
        n = len(s["x"])
        sp = R.reference_specials(n, s["bonds"])
        assert max(len(v) for v in sp.values()) <= 32                    # the engine's special table (MS_MAX)
        per_atom = np.bincount(np.asarray(s["bonds"])[:, 1:].ravel(), minlength=n + 1)
        assert per_atom.max() + s["extra_bond"] <= (8 if hub else 4)     # MAXBPA; <= 4: exclusions come from the bond table
        if hub:
            h = s["hub"]
            assert sum(1 for lv in sp[h].values() if lv == 1) == 6       # more than the four register slots (SPMAX)
    s, x, ref = reference_of("special-hub")
    n = len(x)
    ent = R.expected_entries(ref, np.arange(1, n + 1), n, s["bonds"], (0.0, 0.3, 0.7), (0.0, 0.0, 0.0))
    codes = np.bincount(list(ent.values()), minlength=4)
    assert codes[1] == 0 and codes[2] > 100 and codes[3] > 100 and codes[0] > 1000, codes


@pytest.mark.parametrize("sign", [+1, -1])
def test_trigger_probe_crosses_the_threshold_where_it_says(sign):
    s = I.trigger_probe(sign)
    builds = lambda steps: run_oracle(I.EPS0_SCRIPT + "fix 1 all nve\nrun %d\n" % steps, s).neigh_builds()
    assert builds(I.TRIGGER_STEPS) == I.TRIGGER_BUILDS[sign]
    assert builds(I.TRIGGER_STEPS - 1) == 0 and builds(I.TRIGGER_STEPS + 1) == 1
    # the float copy of the start is off by 1e-4, twice the margin by which the tenth step misses the threshold
    x0 = s["x"][-1, 0]
    err = float(np.float32(x0)) - x0
    d10 = s["v"][-1, 0] * 0.005 * 10
    assert (d10 > 0.2) == (sign < 0) and ((d10 - err) > 0.2) == (sign > 0) and abs(d10 - 0.2) < 0.6e-4 < 0.9e-4 < abs(err)


def test_list_hook_refuses_without_device_state():
    """The hook is exported (not declared in include/lammps_le.h) and answers -1 with the error set before any list exists."""
    import ctypes as CT

    from lammps_le_amd import lammps
    lmp = lammps(cmdargs=["-screen", "none"])
    fn = lmp.lib.lammps_le_test_neighbor_list
    fn.restype = CT.c_longlong
    fn.argtypes = [CT.c_void_p, CT.c_longlong] + [CT.c_void_p] * 6 + [CT.c_longlong] + [CT.c_void_p] * 3
    assert fn(lmp.lmp, 0, None, None, None, None, None, None, 0, None, None, None) == -1
    with pytest.raises(Exception, match="no neighbor list"):
        lmp._check()
    lmp.close()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lammps_le.h")).read()
    assert "lammps_le_test_neighbor_list" not in header


def cell_order(x, box, tile=16):
    """Slot of every bead in the cell order of the list build (bin_inl.h row_id / cell_index; ties by tag)."""
    box = np.asarray(box)
    nc = np.array(I.cell_counts(box))
    c = np.minimum(((x - box[:, 0]) * (nc / (box[:, 1] - box[:, 0]))).astype(int), nc - 1)
    ay, az = c[:, 1], c[:, 2]
    ty, tz = ay // tile, az // tile
    hy, hz = np.minimum(tile, nc[1] - ty * tile), np.minimum(tile, nc[2] - tz * tile)
    row = tz * tile * nc[1] + ty * tile * hz + (az - tz * tile) * hy + (ay - ty * tile)
    return np.lexsort((np.arange(len(x)), row * nc[0] + c[:, 0]))


def test_aligned_rows_have_interior_and_almost_interior_wavefronts():
    s, x, ref = reference_of("aligned-rows")
    box = np.asarray(s["box"])
    assert I.cell_counts(box) == (26, 3, 3) and len(x) % 64 == 0
    order = cell_order(x, box)
    face = np.minimum(x - box[:, 0], box[:, 1] - x).min(axis=1)[order].reshape(-1, 64)       # distance to the nearest face
    interior = (face > C * (1 + 1e-12)).all(axis=1)
    almost = (face > 0.5 * C * (1 + 1e-12)).all(axis=1) & ~interior
    assert interior.sum() == 1 and almost.sum() == 2          # zone 3 / zones 2 and 4 of the middle row
    # beads of the almost-interior wavefronts have neighbors that only the minimum image finds
    raw = np.abs(x[ref.i] - x[ref.j]).max(axis=1) > C
    slot = np.empty(len(x), dtype=int)
    slot[order] = np.arange(len(x))
    wave = slot[ref.i[raw]] // 64
    for w in np.nonzero(almost)[0]:
        assert (wave == w).sum() > 100
    assert not np.isin(wave, np.nonzero(interior)[0]).any()
    assert np.bincount(ref.i).max() > I.initial_maxneigh(len(x), box)
