"""The C-ABI's ID-addressed and compute entry points on the device: subset gather / scatter through kernels_capi.hip
(no whole-system download), on one rank and on in-process slabs, against gather_atoms and the CPU oracle; extract_compute
of the thermo computes and of compute property/local."""
import threading
import uuid

import numpy as np
import pytest

from systems import CHAIN_SCRIPT, OracleScript, run_product, write_data
from test_gpu_le import LE, barrier_types, melted

pytestmark = pytest.mark.gpu

PROPS = ("x", "v", "f", "type", "image", "mask", "molecule", "num_bond", "bond_type", "bond_atom", "nspecial", "special")
N1, ND = 20000, 60000        # one rank; slabs (three slabs of 60k beads are wider than two ghost shells of 6.2)


def _system(n):
    return melted(n, nchains=3, seed=9, types=barrier_types(n, 17))


def _script(sort=False):
    base = CHAIN_SCRIPT.replace("comm_modify cutoff 5.0", "comm_modify cutoff 6.2") \
        .replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 10.0 6.0 1.0 1.0")
    if sort:
        base = base.replace("atom_modify sort 0 0", "atom_modify sort 40 0")
    return base + LE.format(n1=100, nl=100, nu=100, neutral=1, left=2, right=3, tp=0.5, lr="4",
                            lprob="prob 0.5 684474", uprob="prob 0.3 456456", rmax=0.5)


def _ids(seed, n, k):
    rng = np.random.RandomState(seed)
    ids = rng.randint(1, n + 1, size=k).astype(np.int32)
    ids[:3] = ids[3]                      # repeats (and the rest unsorted)
    return ids


def _lines(script, path):
    out = []
    for ln in script.split("\n"):
        w = ln.split("#")[0].split()
        out.append("read_data " + path if w and w[0] == "read_data" else ln)
    return out


def _run_local_ranks(world, script_lines, body):
    """`body(lmp, rank)` on `world` in-process slabs (threads and the transport of test_gpu_dd.run_ranks_local)."""
    from lammps_le_amd import lammps
    session = uuid.uuid4().hex[:12]
    out, errs = [None] * world, []

    def work(rank):
        try:
            lmp = lammps(cmdargs=["-screen", "none"])
            lmp.comm_init("local", rank, world, session=session)
            for ln in script_lines:
                lmp.command(ln)
            out[rank] = body(lmp, rank)
            lmp.close()
        except Exception as e:       # a failing rank leaves the others waiting for the transport's timeout
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    return out


def _packed(im):
    return ((im[:, 0] + 512) & 1023) | (((im[:, 1] + 512) & 1023) << 10) | (((im[:, 2] + 512) & 1023) << 20)


def test_subset_gather_one_rank(tmp_path):
    lmp = run_product(_script() + "run 250\n", _system(N1), tmp_path)
    sets = (_ids(3, N1, 1000), np.arange(N1, 0, -1, dtype=np.int32))       # random with repeats; every ID, reversed
    before = lmp.stat("host_downloads")
    subs = [{name: lmp.gather_ids(name, ids) for name in PROPS} for ids in sets]
    img1 = np.ctypeslib.as_array(lmp.gather_atoms_subset("image", 0, 1, len(sets[0]), list(sets[0]))).copy()
    assert lmp.stat("host_downloads") == before, "a subset gather downloaded the system"
    for ids, sub in zip(sets, subs):
        for name in PROPS:
            assert np.array_equal(sub[name], lmp.gather(name)[ids - 1]), name
    assert np.array_equal(img1, _packed(lmp.gather("image")[sets[0] - 1]))
    lmp.close()


@pytest.mark.parametrize("world", [2, 3])
def test_subset_gather_across_slabs(tmp_path, world):
    path = str(tmp_path / "data.chain")
    write_data(path, _system(ND))
    ids = _ids(4, ND, 700)

    def body(lmp, rank):
        b0, c0 = lmp.stat("host_downloads"), lmp.stat("subset_comm_bytes")
        sub = {name: lmp.gather_ids(name, ids) for name in PROPS}
        stayed = lmp.stat("host_downloads") == b0
        moved = lmp.stat("subset_comm_bytes") - c0
        return stayed, moved, sub, {name: lmp.gather(name) for name in PROPS}

    for stayed, moved, sub, full in _run_local_ranks(world, _lines(_script() + "run 150\n", path), body):
        assert stayed, "a subset gather on slabs downloaded the system"
        for name in PROPS:
            assert np.array_equal(sub[name], full[name][ids - 1]), name
        # O(K): a rank puts K rows + K found flags per per-slot property (x v f image) into the collectives, whatever N is
        assert moved == len(ids) * (3 * (3 * 8 + 4) + (3 * 4 + 4))


def _oracle_after_scatter(script0, s, n, seed):
    o = OracleScript(s).run(script0)
    rng = np.random.RandomState(seed)
    ids = rng.choice(np.arange(1, n + 1), size=300, replace=False).astype(np.int32)
    x, v = o.x(), o.v()
    newx = x[ids - 1] + rng.uniform(-0.05, 0.05, size=(len(ids), 3))
    newv = v[ids - 1] * 0.5 + rng.normal(0.0, 0.1, size=(len(ids), 3))
    x[ids - 1] = newx
    v[ids - 1] = newv
    o.set_x(x)
    o.set_v(v)
    o.run(300)
    return o, ids, newx, newv


def _result(lmp):
    r = dict(bonds=lmp.bond_set(), x=lmp.gather("x"), order=np.ctypeslib.as_array(lmp.gather_atoms_concat("id", 0, 1)).copy())
    for fid in ("loop", "loading", "unloading"):
        r["f_" + fid] = (lmp.extract_fix(fid, 0, 1, 0), lmp.extract_fix(fid, 0, 1, 1))
    return r


def _compare(o, r):
    assert r["bonds"] == o.bond_set()
    assert any(b[0] == 2 for b in r["bonds"]), "the scenario loaded no extruders"
    for fid in ("loop", "loading", "unloading"):
        assert tuple(r["f_" + fid]) == tuple(o.fix_vector(fid)), fid
    err = np.abs(r["x"] - o.x()).max()
    assert err < 1e-9, err
    assert np.array_equal(r["order"], o.local_order())      # the local order the scatter had to keep


@pytest.mark.parametrize("sort", [False, True])
def test_subset_scatter_one_rank_matches_the_oracle(tmp_path, sort):
    s = _system(N1)
    script0 = _script(sort) + "run 100\n"
    o, ids, newx, newv = _oracle_after_scatter(script0, s, N1, 11)
    lmp = run_product(script0, s, tmp_path)
    b0 = lmp.stat("host_downloads")
    lmp.scatter_ids("x", ids, newx)
    lmp.scatter_ids("v", ids, newv)
    assert np.array_equal(lmp.gather_ids("x", ids), newx) and np.array_equal(lmp.gather_ids("v", ids), newv)
    lmp.command("run 300")
    assert lmp.stat("host_downloads") == b0, "a subset scatter took the re-upload path"
    _compare(o, _result(lmp))
    lmp.close()


def test_subset_scatter_three_slabs_matches_the_oracle(tmp_path):
    s = _system(ND)
    script0 = _script() + "run 100\n"
    o, ids, newx, newv = _oracle_after_scatter(script0, s, ND, 12)
    path = str(tmp_path / "data.chain")
    write_data(path, s)

    def body(lmp, rank):
        b0 = lmp.stat("host_downloads")
        lmp.scatter_ids("x", ids, newx)
        lmp.scatter_ids("v", ids, newv)
        lmp.command("run 300")
        return lmp.stat("host_downloads") == b0, _result(lmp)

    for stayed, r in _run_local_ranks(3, _lines(script0, path), body):
        assert stayed, "a subset scatter on slabs took the re-upload path"
        _compare(o, r)


def test_extract_compute_matches_thermo(tmp_path):
    import lammps_le_amd as K
    script = _script() + "thermo_style custom step temp pe press pxx pyy pzz pxy pxz pyz\nthermo_modify norm no\n" \
        "compute bl all property/local btype batom1 batom2\nrun 100\n"
    lmp = run_product(script, _system(N1), tmp_path)
    G = K.LMP_STYLE_GLOBAL

    def check():
        for cid, key in (("thermo_temp", "temp"), ("thermo_pe", "pe"), ("thermo_press", "press")):
            assert lmp.extract_compute(cid, G, K.LMP_TYPE_SCALAR) == lmp.get_thermo(key), cid
        pv = lmp.extract_compute("thermo_press", G, K.LMP_TYPE_VECTOR)
        assert pv == [lmp.get_thermo(k) for k in ("pxx", "pyy", "pzz", "pxy", "pxz", "pyz")]
        tv = lmp.extract_compute("thermo_temp", G, K.LMP_TYPE_VECTOR)
        assert len(tv) == 6 and abs(sum(tv[:3]) / (3 * N1 - 3) - lmp.get_thermo("temp")) < 1e-10
        assert lmp.extract_compute("thermo_pe", G, K.LMP_TYPE_VECTOR) is None
        assert lmp.extract_compute("nope", G, K.LMP_TYPE_SCALAR) is None

    check()
    # a run that ends on a step `thermo 10` does not hit, with a thermo style that no longer prints the tensor
    lmp.command("thermo_style custom step temp pe press")
    lmp.command("run 37")
    check()
    rows = lmp.extract_compute("bl", K.LMP_STYLE_LOCAL, K.LMP_TYPE_ARRAY)
    assert lmp.extract_compute("bl", K.LMP_STYLE_LOCAL, K.LMP_SIZE_ROWS) == len(rows)
    assert lmp.extract_compute("bl", K.LMP_STYLE_LOCAL, K.LMP_SIZE_COLS) == 3
    assert {(int(a), int(b), int(c)) for a, b, c in rows} == lmp.bond_set()
    lmp.close()


def test_gather_concat_gives_the_mapping_of_gather_atoms(tmp_path):
    lmp = run_product(_script(sort=True) + "run 150\n", _system(N1), tmp_path)
    ids = np.ctypeslib.as_array(lmp.gather_atoms_concat("id", 0, 1)).copy()
    xc = np.ctypeslib.as_array(lmp.gather_atoms_concat("x", 1, 3)).reshape(N1, 3).copy()
    assert sorted(ids) == list(range(1, N1 + 1)) and not np.array_equal(ids, np.arange(1, N1 + 1))
    assert np.array_equal(xc, lmp.gather("x")[ids - 1])
    assert np.array_equal(np.ctypeslib.as_array(lmp.gather_atoms_concat("id", 0, 1)), ids)   # same state, same order
    lmp.close()
