"""The rows of compute property/local (natom* / patom*) and compute pair/local on the device, against the brute force of
pair_rows_reference.py: IDs and types exactly, as arrays in (atom1, atom2) order; dist eng force fx fy fz within the
project's ceiling for one evaluation (force_compare.relerr <= 1e-12, floor 1.0).  No state compared here holds an undecided
pair (asserted at the engine's own positions below, and for the oracle's without a GPU in test_pair_rows_cpu.py).

Measured on an MI355X (worst relerr over the six value columns; dist alone stays below 9e-16 everywhere): tiny 4.0e-14,
types 5.4e-14, hubs-harmonic 2.8e-14, offset 1.2e-14, the LE system 5.4e-14, tiny after the subset scatter 5.4e-15, the two
`pair_style zero` inputs 2.5e-16 (dist; eng and force are 0); sum of eng against thermo's evdwl 4.0e-16 at the most;
pair/local of 2 and 3 ranks against the one-rank table 0 on both decomposed inputs."""
import functools
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import pair_rows_reference as PR
from lammps_le_amd import LammpsError
from systems import run_product

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CEILING = 1e-12
NEIGH = "compute n all property/local natom1 natom2 ntype1 ntype2\n"
PAIR = "compute p all property/local patom1 patom2 ptype1 ptype2\ncompute d all pair/local dist eng force fx fy fz\n"
STALE = "Compute used in dump between runs is not current"
_REFERENCES = {}


def reference(name, x, kind, skin="0.4", bonds=None, member=None):
    """pair_rows_reference.reference_rows, computed once per state and shared among the tests (never modified)."""
    key = (name, kind, skin, np.ascontiguousarray(x).tobytes(), None if bonds is None else np.asarray(bonds).tobytes(),
           None if member is None else np.asarray(member).tobytes())
    if key not in _REFERENCES:
        _REFERENCES[key] = PR.reference_rows(name, x, kind, skin, bonds=bonds, member=member)
    rows = _REFERENCES[key]
    assert rows.undecided == []
    return rows


def assert_ids(got, ref, what):
    assert got.shape[0] == len(ref.ids), "%s: %d rows, the reference has %d" % (what, got.shape[0], len(ref.ids))
    assert np.array_equal(got, ref.ids[:, :got.shape[1]].astype(np.float64)), what


def assert_values(got, ref, what):
    worst = 0.0
    for c, k in enumerate(PR.COLUMNS):
        err = PR.relerr(got[:, c], ref.vals[:, c]) if len(got) else 0.0
        print("%s %-5s relerr %.3e" % (what, k, err))
        worst = max(worst, err)
    assert worst <= CEILING, (what, worst)
    return worst


# ---- (1) NEIGH rows at run 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PR.TABLE_INPUTS)
def test_neigh_rows_at_run_0(tmp_path, name):
    lmp = run_product(PR.get(name)["head"]("0.4") + NEIGH + "run 0\n", PR.get(name)["system"], tmp_path)
    before = lmp.stat("host_downloads")
    got = lmp.pair_rows("n")
    assert lmp.stat("host_downloads") == before
    ref = reference(name, lmp.gather("x"), "neigh")
    print("%s: %d NEIGH rows" % (name, len(got)))
    assert_ids(got, ref, name)
    assert lmp.stat("pair_rows") == len(got) and 2 * len(got) == lmp.stat("neigh_pairs")
    if name == "dense_cluster":          # hundreds of rows behind one bead: the per-bead ordering
        assert np.bincount(got[:, 0].astype(np.int64)).max() > 250
    lmp.close()


# ---- (2) PAIR rows and pair/local after a few steps ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", PR.FORCE_INPUTS)
def test_pair_rows_after_steps(tmp_path, name):
    """STEPS steps of fix nve, the last one on the list of an earlier step: rows by the CURRENT separations.
    Worst relerr of a value column measured on an MI355X: see the module docstring."""
    s = PR.get(name)["system"]
    lmp = run_product(PR.steps_script(name, PR.STEPS, extra=PAIR), s, tmp_path)
    passes, downloads = lmp.stat("pair_row_passes"), lmp.stat("host_downloads")
    p, d = lmp.pair_rows("p"), lmp.pair_rows("d")
    assert lmp.stat("pair_row_passes") == passes + 1, "the two computes share one device pass"
    assert lmp.stat("host_downloads") == downloads
    x = lmp.gather("x")
    ref = reference(name, x, "pair", "0.2")
    assert_ids(p, ref, name)
    assert d.shape == (len(ref.ids), 6)
    assert_values(d, ref, name)
    evdwl = lmp.get_thermo("evdwl") * len(x)          # (thermo_modify norm yes)
    err = PR.relerr(d[:, 1].sum(), evdwl)
    print("%s: %d PAIR rows, sum(eng) %.15g, thermo evdwl %.15g, relerr %.3e" % (name, len(p), d[:, 1].sum(), evdwl, err))
    assert err <= CEILING
    assert PR.relerr(ref.vals[:, 1].sum(), evdwl) <= CEILING
    if name == "types":          # the cutoffs between 1.12 and 2.5 all decide rows (no 1-2 pair is within its cutoff of 1.0)
        t = np.sort(p[:, 2:].astype(np.int64), axis=1)
        assert {tuple(r) for r in t.tolist()} >= {(1, 1), (1, 3), (2, 2), (2, 3), (3, 3)}
        assert all(d[k, 1] == 0.0 and d[k, 2] == 0.0 for k in np.nonzero((t[:, 0] == 1) & (t[:, 1] == 2))[0])
    lmp.close()


@pytest.mark.parametrize("name", ["dense_cluster", "slab_ladder"])
def test_pair_rows_of_pair_style_zero(tmp_path, name):
    """`pair_style zero 1.12`: rows by its cutoff, eng and force 0, dist as measured."""
    lmp = run_product(PR.get(name)["head"]("0.4") + PAIR + "run 0\n", PR.get(name)["system"], tmp_path)
    p, d = lmp.pair_rows("p"), lmp.pair_rows("d")
    ref = reference(name, lmp.gather("x"), "pair")
    assert_ids(p, ref, name)
    assert_values(d, ref, name)
    assert not d[:, 1:].any() and (d[:, 0] > 0).all() and (d[:, 0] < 1.12).all()
    lmp.close()


# ---- (3) a compute on a group ---------------------------------------------------------------------------------------------------
def test_rows_of_a_group(tmp_path):
    name = "hubs-harmonic"
    s = PR.get(name)["system"]
    n = len(s["x"])
    extra = PAIR + "group odd id 1:%d:2\ngroup low id 1:%d\ncompute po odd property/local patom1 patom2\ncompute do odd pair/local eng fz\n" % (n, n // 3)
    lmp = run_product(PR.steps_script(name, PR.STEPS, extra=extra), s, tmp_path)
    po, do, p = lmp.pair_rows("po"), lmp.pair_rows("do"), lmp.pair_rows("p")
    x = lmp.gather("x")
    odd = np.arange(1, n + 1) % 2 == 1
    ref = reference(name, x, "pair", "0.2", member=odd)
    assert_ids(po, ref, "odd")
    assert 0 < len(po) < len(p) and (po % 2 == 1).all()
    assert PR.relerr(do[:, 0], ref.vals[:, 1]) <= CEILING and PR.relerr(do[:, 1], ref.vals[:, 5]) <= CEILING
    # computes defined after the run, on a group no compute or fix named before it: the masks follow without a run in between
    lmp.command("compute nl low property/local natom1 natom2")
    lmp.command("compute pl low property/local patom1 patom2")
    downloads = lmp.stat("host_downloads")
    pl = lmp.pair_rows("pl")
    assert lmp.stat("host_downloads") == downloads
    assert_ids(pl, reference(name, x, "pair", "0.2", member=np.arange(1, n + 1) <= n // 3), "low")
    assert len(pl) > 0 and pl.max() <= n // 3 and len(lmp.pair_rows("nl")) > len(pl)
    lmp.close()


# ---- (4) a firing of fix ex_load ----------------------------------------------------------------------------------------------------
def test_new_extruder_bonds_leave_the_rows(tmp_path):
    name = "le_small"
    s = PR.get(name)["system"]
    lmp = run_product(PR.steps_script(name, PR.LE_STEPS, extra=PAIR), s, tmp_path)
    p, d = lmp.pair_rows("p"), lmp.pair_rows("d")
    x = lmp.gather("x")
    bonds = np.array(sorted(lmp.bond_set()), dtype=np.int64)
    new = [tuple(b[1:]) for b in bonds.tolist() if b[0] == 2]
    ref = reference(name, x, "pair", "0.4", bonds=bonds)
    assert_ids(p, ref, name)
    assert_values(d, ref, name)
    before = reference(name, x, "pair", "0.4")          # the same positions under the data file's bonds
    had, has = set(map(tuple, before.ids[:, :2].tolist())), set(map(tuple, p[:, :2].astype(np.int64).tolist()))
    print("new extruder bonds %d, inside the pair cutoff %d" % (len(new), sum(1 for b in new if b in had)))
    assert len(new) >= 3 and sum(1 for b in new if b in had) >= 3 and not any(b in has for b in new)
    lmp.close()


# ---- (5) z slabs ------------------------------------------------------------------------------------------------------------------------
def dd_script(name):
    if PR.DD_INPUTS[name] == 0:
        return PR.get(name)["head"]("0.4") + NEIGH + PAIR + "run 0\n", ("n", "p", "d")
    return PR.steps_script(name, PR.DD_INPUTS[name], extra=PAIR), ("p", "d")


def run_in_children(world, system, script, ids, tmp_path):
    session = uuid.uuid4().hex[:12]
    sysfile, scriptfile, out = (os.path.join(str(tmp_path), n) for n in ("system.pkl", "script.txt", "out"))
    pickle.dump(system, open(sysfile, "wb"))
    open(scriptfile, "w").write(script)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "pair_rows_worker.py"), str(r), str(world), session, sysfile,
                               scriptfile, out, ",".join(ids)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [dict(np.load("%s.r%d.npz" % (out, r))) for r in range(world)]


@functools.lru_cache(maxsize=None)
def one_rank_tables(name, tmp):
    script, ids = dd_script(name)
    lmp = run_product(script, PR.get(name)["system"], tmp)
    out = {cid: lmp.pair_rows(cid) for cid in ids}
    out["x"] = lmp.gather("x")
    lmp.close()
    return out


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", sorted(PR.DD_INPUTS))
def test_decomposed_tables_equal_the_one_rank_table(tmp_path_factory, tmp_path, name, world):
    s = PR.get(name)["system"]
    one = one_rank_tables(name, str(tmp_path_factory.mktemp("one_rank_" + name)))
    ref = reference(name, one["x"], "pair", "0.4" if PR.DD_INPUTS[name] == 0 else "0.2")
    assert_ids(one["p"], ref, name + " on one rank")
    script, ids = dd_script(name)
    ranks = run_in_children(world, s, script, ids, tmp_path)
    assert all(r["nlocal"][0] > 0 for r in ranks) and sum(r["nlocal"][0] for r in ranks) == len(s["x"])
    for k, r in enumerate(ranks):
        assert r["downloads"][0] == r["downloads"][1], "an extract downloaded the system"
        for cid in ids:
            got, want = r["rows_" + cid], one[cid]
            assert got.shape == want.shape, (name, world, k, cid, got.shape, want.shape)
            if cid == "d":
                err = max(PR.relerr(got[:, c], want[:, c]) for c in range(6))
                print("%s, %d ranks, rank %d: pair/local against the one-rank table, relerr %.3e" % (name, world, k, err))
                assert err <= CEILING
            else:
                assert np.array_equal(got, want), (name, world, k, cid)
            assert np.array_equal(got, ranks[0]["rows_" + cid]), "the ranks' tables differ"
    # pairs across a slab face: there are some, and each is in the table once
    box = np.asarray(s["box"], dtype=np.float64)
    z = ranks[0]["x"][:, 2]
    owner = np.clip(((z - box[2, 0]) / ((box[2, 1] - box[2, 0]) / world)).astype(np.int64), 0, world - 1)
    p = ranks[0]["rows_p"][:, :2].astype(np.int64)
    across = int((owner[p[:, 0] - 1] != owner[p[:, 1] - 1]).sum())
    print("%s, %d ranks: %d rows, %d of them across a slab face" % (name, world, len(p), across))
    assert across >= 10 and len(set(map(tuple, p.tolist()))) == len(p)


# ---- (6) dump local --------------------------------------------------------------------------------------------------------------------------
def test_dump_local_writes_the_extracted_rows(tmp_path):
    name = "tiny"
    s = PR.get(name)["system"]
    dump = "dump 1 all local %d %s index c_p[1] c_p[2] c_d[1] c_d[2]\n" % (PR.STEPS, tmp_path / "pairs.*.dump")
    lmp = run_product(PR.steps_script(name, PR.STEPS, extra=PAIR + dump), s, tmp_path)
    assert lmp.stat("host_downloads") == 0, "a dump of pair rows alone needs no host copy of the system"
    p, d = lmp.pair_rows("p"), lmp.pair_rows("d")
    text = open(str(tmp_path / ("pairs.%d.dump" % PR.STEPS))).read().split("\n")
    assert text[0] == "ITEM: TIMESTEP" and int(text[1]) == PR.STEPS
    assert text[2] == "ITEM: NUMBER OF ENTRIES" and int(text[3]) == len(p)
    assert text[8] == "ITEM: ENTRIES index c_p[1] c_p[2] c_d[1] c_d[2]"
    body = [ln.split() for ln in text[9:9 + len(p)]]
    assert text[9 + len(p):] == [""]
    for r, words in enumerate(body):
        assert words == ["%d" % (r + 1), "%g" % p[r, 0], "%g" % p[r, 1], "%g" % d[r, 0], "%g" % d[r, 1]], r
    assert os.path.exists(str(tmp_path / "pairs.0.dump"))
    # a dump local without any compute column still lists the bonds, one row each
    lmp.command("undump 1")
    lmp.command("dump 3 all local 1 %s index" % (tmp_path / "index.*.dump"))
    lmp.command("run 0")
    only = open(str(tmp_path / ("index.%d.dump" % PR.STEPS))).read().split("\n")
    assert int(only[3]) == len(s["bonds"]) and only[9:9 + len(s["bonds"])] == ["%d" % (r + 1) for r in range(len(s["bonds"]))]
    lmp.command("undump 3")
    lmp.close()
    # columns with different row counts: NEIGH kind beside pair/local, and two groups
    for extra in (NEIGH + PAIR + "dump 2 all local 5 %s c_n[1] c_d[1]\n" % (tmp_path / "bad.dump"),
                  PAIR + "group odd id 1:83:2\ncompute po odd property/local patom1\ndump 2 all local 5 %s c_p[1] c_po[1]\n" % (tmp_path / "bad.dump")):
        from lammps_le_amd import lammps
        bad = lammps(cmdargs=["-screen", "none"])
        try:
            lines = PR.steps_script(name, PR.STEPS, extra=extra).replace("read_data data.force", "read_data %s" % (tmp_path / "data.force")).split("\n")
            with pytest.raises(LammpsError, match="Dump local count is not consistent across input fields"):
                for ln in lines:
                    bad.command(ln)
        finally:
            bad.close()


# ---- (7) no download; a subset scatter at the same timestep ------------------------------------------------------------------------------------
def test_subset_scatter_changes_the_pair_rows(tmp_path):
    name = "tiny"
    s = PR.get(name)["system"]
    lmp = run_product(PR.get(name)["head"]("0.4") + "group low id 1:40\n" + NEIGH + PAIR + "run 0\n", s, tmp_path)
    downloads = lmp.stat("host_downloads")
    p0, d0, n0 = lmp.pair_rows("p"), lmp.pair_rows("d"), lmp.pair_rows("n")
    # a compute on a group that nothing named when the run began: its bits reach the device with the first extract
    lmp.command("compute pl low property/local patom1 patom2")
    pl = lmp.pair_rows("pl")
    assert lmp.stat("host_downloads") == downloads
    x = lmp.gather("x")
    assert_ids(p0, reference(name, x, "pair"), name)
    assert_ids(pl, reference(name, x, "pair", member=np.arange(1, len(x) + 1) <= 40), "low")
    assert 0 < len(pl) < len(p0)
    a, b, pos = PR.nudge(name, x)
    assert [a, b] in p0[:, :2].astype(np.int64).tolist()
    passes = lmp.stat("pair_row_passes")
    assert np.array_equal(lmp.pair_rows("p"), p0) and lmp.stat("pair_row_passes") == passes          # (cached)
    lmp.scatter_ids("x", [a], pos.reshape(1, 3))          # same timestep, no run in between
    p1, d1 = lmp.pair_rows("p"), lmp.pair_rows("d")
    assert lmp.stat("pair_row_passes") == passes + 1
    x1 = x.copy()
    x1[a - 1] = pos
    ref = reference(name, x1, "pair")
    assert_ids(p1, ref, "after the scatter")
    assert_values(d1, ref, "after the scatter")
    assert [a, b] not in p1[:, :2].astype(np.int64).tolist() and len(p1) < len(p0)
    assert np.array_equal(lmp.pair_rows("n"), n0), "the NEIGH rows are the list's, whatever moved since"
    lmp.close()


# ---- (8) a whole-system scatter ----------------------------------------------------------------------------------------------------------------
def test_whole_system_scatter_makes_the_extract_refuse(tmp_path):
    name = "tiny"
    s = PR.get(name)["system"]
    lmp = run_product(PR.get(name)["head"]("0.4") + NEIGH + PAIR + "compute b all property/local btype batom1 batom2\nrun 0\n", s, tmp_path)
    p0 = lmp.pair_rows("p")
    x = lmp.gather("x")
    lmp.scatter("x", x)          # the host copies are the state now
    for cid in ("n", "p", "d"):
        with pytest.raises(LammpsError, match=STALE):
            lmp.pair_rows(cid)
        with pytest.raises(LammpsError, match=STALE):
            lmp.extract_compute(cid, 2, 4)
    assert len(lmp.pair_rows("b")) == len(s["bonds"])          # the bond attributes answer from the host tables, as before
    lmp.command("run 0")
    assert np.array_equal(lmp.pair_rows("p"), p0)
    # a compute defined since the last run meets its init() checks when it is first asked
    lmp.command("compute x1 all pair/local dist p1")
    with pytest.raises(LammpsError, match="Pair style does not have extra field requested by compute pair/local"):
        lmp.pair_rows("x1")
    lmp.close()
