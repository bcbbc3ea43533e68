"""CPU checks of the binding set python/lammps.py expects (its constructor binds 55 lammps_* entry points without a guard)
and of the entry points that need no device: variables, IDs, styles, datatypes, reset_box, the out-of-scope calls that
record an error, and the subset calls on the host copies before the first run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from systems import CHAIN_SCRIPT, lattice_chain, write_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from lammps_le_amd import library_path
    return C.CDLL(library_path())


def test_every_name_the_reference_python_module_binds_is_exported():
    """The names python/lammps.py's constructor sets argtypes / restype on, in the way it does it."""
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "lammps_py_bindings.json")))
    assert len(names) == 55
    lib = _lib()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    for n in names:
        fn = getattr(lib, n)
        fn.argtypes = [C.c_void_p]
        fn.restype = C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "lammps_le.h")).read()
    for n in names:
        assert n + "(" in hdr, n


def _open(tmp_path, n=300, log=None):
    from lammps_le_amd import lammps
    s = lattice_chain(n)
    path = os.path.join(str(tmp_path), "data.chain")
    write_data(path, s)
    lmp = lammps(cmdargs=["-screen", "none"] + (["-log", log] if log else []))
    for ln in CHAIN_SCRIPT.split("\n"):
        lmp.command(ln.replace("data.chain", path))
    return lmp, s


def test_variables(tmp_path):
    lmp, _ = _open(tmp_path)
    lmp.command("variable a equal 2*3+1")
    lmp.command("variable s string hello")
    lmp.command("variable i index first second")
    lmp.command("variable l loop 3")
    assert lmp.extract_variable("a") == 7.0
    assert lmp.extract_variable("s") == "hello"
    assert lmp.extract_variable("i") == "first"
    assert lmp.extract_variable("l") == "1"
    assert lmp.extract_variable("nope") is None
    assert lmp.set_variable("s", "world") == 0
    assert lmp.extract_variable("s") == "world"
    lmp.command("variable b equal v_a*2")
    assert lmp.extract_variable("b") == 14.0
    assert lmp.set_variable("a", "5") == -1           # not a string-style variable
    assert lmp.set_variable("nope", "5") == -1
    assert lmp.extract_variable("a") == 7.0


def test_ids_styles_and_datatypes(tmp_path):
    import lammps_le_amd as K
    lmp, _ = _open(tmp_path)
    lmp.command("group low id 1:50")
    lmp.command("region box1 block 0 5 0 5 0 5")
    lmp.command("fix 1 all nve")
    lmp.command("variable a equal 1")
    lmp.command("compute bl all property/local btype batom1 batom2")
    assert lmp.has_id("group", "low") and lmp.has_id("group", "all") and not lmp.has_id("group", "high")
    assert lmp.has_id("region", "box1") and lmp.has_id("fix", "1") and lmp.has_id("variable", "a")
    assert lmp.has_id("compute", "bl") and lmp.has_id("compute", "thermo_temp")
    assert not lmp.has_id("molecule", "x") and lmp.id_count("molecule") == 0
    assert lmp.available_ids("group") == ["all", "low"]
    assert lmp.available_ids("fix") == ["1"] and lmp.id_count("region") == 1
    assert set(lmp.available_ids("compute")) == {"thermo_temp", "thermo_press", "thermo_pe", "bl"}
    lib, h = lmp.lib, lmp.lmp
    lib.lammps_style_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(64)
    for cat in (b"atom", b"bond", b"compute", b"dump", b"fix", b"pair"):
        n = lib.lammps_style_count(h, cat)
        assert n > 0
        names = []
        for i in range(n):
            assert lib.lammps_style_name(h, cat, i, buf, 64) == 1
            names.append(buf.value.decode())
            assert lmp.has_style(cat.decode(), names[-1])
        assert lib.lammps_style_name(h, cat, n, buf, 64) == 0 and buf.value == b""
    assert lib.lammps_style_count(h, b"kspace") == 0
    assert "extrusion" in [s for s in lmp.available_styles("fix")]
    lib.lammps_extract_global_datatype.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_extract_atom_datatype.argtypes = [C.c_void_p, C.c_char_p]
    for name, dt in (("dt", K.LAMMPS_DOUBLE), ("ntimestep", K.LAMMPS_INT64), ("natoms", K.LAMMPS_INT64),
                     ("boxlo", K.LAMMPS_DOUBLE), ("ntypes", K.LAMMPS_INT), ("units", K.LAMMPS_STRING), ("nope", -1)):
        assert lib.lammps_extract_global_datatype(h, name.encode()) == dt, name
    for name, dt in (("x", K.LAMMPS_DOUBLE_2D), ("v", K.LAMMPS_DOUBLE_2D), ("type", K.LAMMPS_INT), ("id", K.LAMMPS_INT),
                     ("mass", K.LAMMPS_DOUBLE), ("image", K.LAMMPS_INT), ("nope", -1)):
        assert lib.lammps_extract_atom_datatype(h, name.encode()) == dt, name
    pk = []
    for i in range(8):
        if lib.lammps_config_package_name(i, buf, 64):
            pk.append(buf.value.decode())
    assert "USER-LE" in pk and "MOLECULE" in pk and "MC" in pk
    lib.lammps_get_os_info.argtypes = [C.c_char_p, C.c_int]
    big = C.create_string_buffer(512)
    lib.lammps_get_os_info(big, 512)
    assert len(big.value) > 0
    lib.lammps_get_mpi_comm.argtypes = [C.c_void_p]
    assert lib.lammps_get_mpi_comm(h) == -1


def test_reset_box_without_a_box_warns(tmp_path):
    from lammps_le_amd import lammps
    log = os.path.join(str(tmp_path), "log.lammps")
    lmp = lammps(cmdargs=["-screen", "none", "-log", log])
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(5, 5, 5)
    lmp.lib.lammps_reset_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double]
    lmp.lib.lammps_reset_box(lmp.lmp, lo, hi, 0.0, 0.0, 0.0)
    assert not lmp.lib.lammps_has_error(lmp.lmp)
    lmp.close()
    assert "WARNING: Calling lammps_reset_box without a box" in open(log).read()


def test_reset_box_sets_the_box(tmp_path):
    lmp, s = _open(tmp_path)
    (lo0, hi0, *_) = lmp.extract_box()
    lo, hi = (C.c_double * 3)(*[a - 1.0 for a in lo0]), (C.c_double * 3)(*[b + 1.0 for b in hi0])
    lmp.lib.lammps_reset_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double]
    lmp.lib.lammps_reset_box(lmp.lmp, lo, hi, 0.0, 0.0, 0.0)
    (lo1, hi1, *_) = lmp.extract_box()
    assert np.allclose(lo1, np.array(lo0) - 1.0) and np.allclose(hi1, np.array(hi0) + 1.0)


def test_out_of_scope_calls_record_their_error(tmp_path):
    from lammps_le_amd import LammpsError
    lmp, _ = _open(tmp_path)
    lib, h = lmp.lib, lmp.lmp
    buf = C.create_string_buffer(256)
    lib.lammps_find_pair_neighlist.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    lib.lammps_find_fix_neighlist.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.lammps_find_compute_neighlist.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.lammps_neighlist_num_elements.argtypes = [C.c_void_p, C.c_int]
    lib.lammps_neighlist_element_neighbors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    calls = [(lambda: lib.lammps_find_pair_neighlist(h, b"lj/cut", 1, 0, 0), -1),
             (lambda: lib.lammps_find_fix_neighlist(h, b"1", 0), -1),
             (lambda: lib.lammps_find_compute_neighlist(h, b"c", 0), -1),
             (lambda: lib.lammps_neighlist_num_elements(h, 0), 0)]
    for call, ret in calls:
        assert call() == ret
        assert lib.lammps_has_error(h) == 1
        lib.lammps_get_last_error_message(h, buf, 256)
        assert buf.value.decode() == "neighbor list access is not supported"
    ia, nn, nb = C.c_int(7), C.c_int(7), C.c_void_p(1)
    lib.lammps_neighlist_element_neighbors(h, 0, 0, C.byref(ia), C.byref(nn), C.byref(nb))
    assert lib.lammps_has_error(h) == 1 and ia.value == -1 and nn.value == 0 and not nb.value
    lib.lammps_get_last_error_message(h, buf, 256)
    lib.lammps_set_fix_external_callback.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
    lib.lammps_fix_external_set_energy_global.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    lib.lammps_fix_external_set_virial_global.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    vir = (C.c_double * 6)()
    for call in (lambda: lib.lammps_set_fix_external_callback(h, b"ext", None, None),
                 lambda: lib.lammps_fix_external_set_energy_global(h, b"ext", 1.0),
                 lambda: lib.lammps_fix_external_set_virial_global(h, b"ext", vir)):
        call()
        assert lib.lammps_has_error(h) == 1
        lib.lammps_get_last_error_message(h, buf, 256)
        assert buf.value.decode() == "Can not find fix with ID 'ext'!"
    # the Python mirror raises the recorded error on the next checked call
    lib.lammps_find_fix_neighlist(h, b"1", 0)
    with pytest.raises(LammpsError, match="neighbor list access is not supported"):
        lmp._check()


def _packed(im):
    return ((im[:, 0] + 512) & 1023) | (((im[:, 1] + 512) & 1023) << 10) | (((im[:, 2] + 512) & 1023) << 20)


def test_subset_calls_on_the_host_copies(tmp_path):
    """Before the first run the host copies are the state: the subset calls read and write them, in caller order."""
    from lammps_le_amd import LammpsError
    lmp, s = _open(tmp_path)
    n = lmp.get_natoms()
    ids = np.array([5, 1, 300, 5, 17], dtype=np.int32)
    x = lmp.gather("x")
    assert np.array_equal(lmp.gather_ids("x", ids), x[ids - 1])
    for name in ("type", "id", "mask", "molecule", "image", "num_bond", "bond_type", "bond_atom", "nspecial", "special"):
        assert np.array_equal(lmp.gather_ids(name, ids), lmp.gather(name)[ids - 1]), name
    packed = _packed(lmp.gather("image")[ids - 1])
    got = np.ctypeslib.as_array(lmp.gather_atoms_subset("image", 0, 1, len(ids), list(ids)))
    assert np.array_equal(got, packed)
    newx = x[ids - 1] + 0.25
    lmp.scatter_ids("x", ids, newx)                   # ID 5 twice: its last row stays
    x2 = lmp.gather("x")
    assert np.array_equal(x2[ids - 1][1:], newx[1:]) and np.array_equal(x2[4], newx[3])
    lmp.scatter_ids("image", [7, 9], [[1, -2, 3], [0, 0, -1]])
    assert lmp.gather("image")[6].tolist() == [1, -2, 3] and lmp.gather("image")[8].tolist() == [0, 0, -1]
    im = np.array([[4, 5, -6]])
    lmp.scatter_atoms_subset("image", 0, 1, 1, [11], (C.c_int * 1)(int(_packed(im)[0])))
    assert lmp.gather("image")[10].tolist() == [4, 5, -6]
    with pytest.raises(LammpsError, match="lammps_gather_atoms_subset: unknown atom ID 0"):
        lmp.gather_ids("x", [1, 0])
    with pytest.raises(LammpsError, match="unknown atom ID %d" % (n + 1)):
        lmp.scatter_ids("x", [n + 1], [[0.0, 0.0, 0.0]])
    with pytest.raises(LammpsError, match="lammps_gather_atoms_subset: unknown property name q"):
        lmp.gather_atoms_subset("q", 1, 1, 1, [1])
    # the atom-property forms reject per-atom names of fixes, computes and custom properties
    for fn in ("lammps_gather", "lammps_gather_concat"):
        data = (C.c_double * (3 * n))()
        getattr(lmp.lib, fn)(lmp.lmp, b"f_1", 1, 3, data)
        with pytest.raises(LammpsError, match=fn + ": unknown property name f_1"):
            lmp._check()
    data = (C.c_double * (3 * n))()
    lmp.lib.lammps_gather(lmp.lmp, b"x", 1, 3, data)
    lmp._check()
    assert np.array_equal(np.ctypeslib.as_array(data).reshape(n, 3), lmp.gather("x"))
    # concat: the local order, which is the ID order while no Atom::sort has run
    assert np.array_equal(np.ctypeslib.as_array(lmp.gather_atoms_concat("id", 0, 1)), np.arange(1, n + 1))
    assert lmp.stat("host_downloads") == 0


def test_force_timeout_skips_the_next_run(tmp_path):
    lmp, _ = _open(tmp_path)
    lmp.force_timeout()
    lmp.command("run 10")            # src/run.cpp:47: returns at once, no device needed
    p = lmp.lib.lammps_extract_global(lmp.lmp, b"ntimestep")
    assert C.cast(p, C.POINTER(C.c_long))[0] == 0
