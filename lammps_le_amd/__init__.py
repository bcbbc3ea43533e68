"""lammps_le_amd — MI355X-native engine for the bead-spring + loop-extrusion hot path of
polly-code/lammps_le, behind the reference's own interfaces.

`lammps` mirrors the subset of the reference's ctypes wrapper (python/lammps.py) that drives this
path: same method names and argument meaning, on top of the C-ABI in include/lammps_le.h
(liblammps_le.so, hand-written HIP for gfx950).  There is NO CPU fallback: `run` fails loudly
without a HIP device, and importing fails loudly if the shared library has not been built.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liblammps_le.so")
if os.environ.get("LAMMPS_LE_LIBRARY"):      # development only: A/B runs of two builds of the engine (scripts/run_ab.sh)
    _SO = os.path.abspath(os.environ["LAMMPS_LE_LIBRARY"])

__all__ = ["lammps", "LammpsError", "library_path", "comm_unique_id", "init_from_torch_distributed"]


class LammpsError(Exception):
    pass


# data types of lammps_extract_global_datatype / lammps_extract_atom_datatype (src/library.h:47-55) and the style / type
# selectors of lammps_extract_compute (:61-78)
LAMMPS_INT, LAMMPS_INT_2D, LAMMPS_DOUBLE, LAMMPS_DOUBLE_2D, LAMMPS_INT64, LAMMPS_INT64_2D, LAMMPS_STRING = range(7)
LMP_STYLE_GLOBAL, LMP_STYLE_ATOM, LMP_STYLE_LOCAL = range(3)
LMP_TYPE_SCALAR, LMP_TYPE_VECTOR, LMP_TYPE_ARRAY, LMP_SIZE_VECTOR, LMP_SIZE_ROWS, LMP_SIZE_COLS = range(6)


# lammps_le_stat "min_stop" indexes these: the reference's Min::stopstrings, as the engine prints them in its stats block (the
# tests read the printed text back through this table, so the two cannot drift apart unnoticed)
MIN_STOP_STRINGS = ("max iterations", "max force evaluations", "energy tolerance", "force tolerance", "search direction is not downhill",
                    "linesearch alpha is zero", "forces are zero", "quadratic factors are zero", "trust region too small",
                    "HFTN minimizer error", "walltime limit reached", "max iterations with v.f negative")


def library_path():
    return _SO


def _load():
    if not os.path.exists(_SO):
        raise ImportError(
            "lammps_le_amd: %s is missing — build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C lammps_le_amd/csrc)" % _SO)
    lib = C.CDLL(_SO, mode=C.RTLD_GLOBAL)
    lib.lammps_open_no_mpi.restype = C.c_void_p
    lib.lammps_open_no_mpi.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p]
    lib.lammps_close.argtypes = [C.c_void_p]
    lib.lammps_file.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_command.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_command.restype = C.c_char_p
    lib.lammps_commands_string.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_get_natoms.argtypes = [C.c_void_p]
    lib.lammps_get_natoms.restype = C.c_double
    lib.lammps_get_thermo.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_get_thermo.restype = C.c_double
    lib.lammps_extract_setting.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_extract_setting.restype = C.c_int
    lib.lammps_extract_global.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_extract_global.restype = C.c_void_p
    lib.lammps_extract_atom.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_extract_atom.restype = C.c_void_p
    lib.lammps_extract_fix.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.lammps_extract_fix.restype = C.c_void_p
    lib.lammps_gather_atoms.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    lib.lammps_scatter_atoms.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    lib.lammps_extract_box.argtypes = [C.c_void_p] + [C.c_void_p] * 7
    lib.lammps_free.argtypes = [C.c_void_p]
    lib.lammps_has_error.argtypes = [C.c_void_p]
    lib.lammps_get_last_error_message.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.lammps_has_style.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.lammps_le_stat.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_le_stat.restype = C.c_double
    for fn in ("lammps_gather_atoms_subset", "lammps_scatter_atoms_subset", "lammps_gather_subset", "lammps_scatter_subset"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    for fn in ("lammps_gather_atoms_concat", "lammps_gather_concat", "lammps_gather", "lammps_scatter"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    lib.lammps_extract_compute.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    lib.lammps_extract_compute.restype = C.c_void_p
    lib.lammps_extract_variable.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.lammps_extract_variable.restype = C.c_void_p
    lib.lammps_extract_variable_datatype.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_set_variable.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.lammps_set_variable.restype = C.c_int
    lib.lammps_has_id.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.lammps_id_count.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_id_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.lammps_force_timeout.argtypes = [C.c_void_p]
    lib.lammps_style_count.argtypes = [C.c_void_p, C.c_char_p]
    lib.lammps_style_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    return lib


class lammps(object):
    """Counterpart of python/lammps.py `lammps` for this path (1 rank per process, one GPU per rank)."""

    def __init__(self, name="", cmdargs=None, ptr=None, comm=None):
        self.lib = _load()
        args = ["lammps"] + list(cmdargs or [])
        argv = (C.c_char_p * len(args))(*[a.encode() for a in args])
        self.lmp = C.c_void_p(self.lib.lammps_open_no_mpi(len(args), argv, None))
        if not self.lmp:
            raise LammpsError("could not create engine instance")
        self.opened = 1

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "opened", 0):
            self.lib.lammps_close(self.lmp)
            self.opened = 0
            self.lmp = None

    # -- error plumbing: python/lammps.py raises on lammps_has_error when built with exceptions --
    def _check(self):
        if self.lib.lammps_has_error(self.lmp):
            buf = C.create_string_buffer(512)
            self.lib.lammps_get_last_error_message(self.lmp, buf, 512)
            raise LammpsError(buf.value.decode())

    def version(self):
        return self.lib.lammps_version(self.lmp)

    def file(self, path):
        self.lib.lammps_file(self.lmp, path.encode())
        self._check()

    def command(self, cmd):
        self.lib.lammps_command(self.lmp, cmd.encode())
        self._check()

    def commands_list(self, cmdlist):
        for c in cmdlist:
            self.command(c)

    def commands_string(self, multicmd):
        self.lib.lammps_commands_string(self.lmp, multicmd.encode())
        self._check()

    def get_natoms(self):
        return int(self.lib.lammps_get_natoms(self.lmp))

    def get_thermo(self, name):
        v = self.lib.lammps_get_thermo(self.lmp, name.encode())
        self._check()
        return v

    def extract_setting(self, name):
        return self.lib.lammps_extract_setting(self.lmp, name.encode())

    def extract_box(self):
        lo = (C.c_double * 3)()
        hi = (C.c_double * 3)()
        xy, yz, xz = C.c_double(), C.c_double(), C.c_double()
        pf = (C.c_int * 3)()
        bf = C.c_int()
        self.lib.lammps_extract_box(self.lmp, lo, hi, C.byref(xy), C.byref(yz), C.byref(xz), pf, C.byref(bf))
        return list(lo), list(hi), xy.value, yz.value, xz.value, list(pf), bf.value

    def extract_fix(self, fid, style, type, nrow=0, ncol=0):
        p = self.lib.lammps_extract_fix(self.lmp, fid.encode(), style, type, nrow, ncol)
        self._check()
        if not p:
            return None
        val = C.cast(p, C.POINTER(C.c_double))[0]
        self.lib.lammps_free(p)
        return val

    def gather_atoms(self, name, type, count):
        """As python/lammps.py: returns a ctypes array of natoms*count values ordered by atom ID."""
        n = self.get_natoms()
        data = ((C.c_double if type == 1 else C.c_int) * (n * count))()
        self.lib.lammps_gather_atoms(self.lmp, name.encode(), type, count, data)
        self._check()
        return data

    def scatter_atoms(self, name, type, count, data):
        self.lib.lammps_scatter_atoms(self.lmp, name.encode(), type, count, data)
        self._check()

    # -- numpy conveniences (python/lammps.py has the same idea in lammps.numpy) --
    def gather(self, name):
        ints = {"type": 1, "id": 1, "mask": 1, "molecule": 1, "image": 3, "num_bond": 1, "nspecial": 3, "num_angle": 1}
        n = self.get_natoms()
        if name in ("x", "v", "f"):
            return np.ctypeslib.as_array(self.gather_atoms(name, 1, 3)).reshape(n, 3).copy()
        if name in ("bond_type", "bond_atom"):
            w = self.extract_setting("bond_per_atom")
        elif name == "special":
            w = self.extract_setting("maxspecial")
        elif name in ("angle_type", "angle_atom1", "angle_atom2", "angle_atom3"):
            w = self.extract_setting("angle_per_atom")
        else:
            w = ints[name]
        a = np.ctypeslib.as_array(self.gather_atoms(name, 0, w)).reshape(n, w).copy()
        return a[:, 0] if w == 1 else a

    def scatter(self, name, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64 if name in ("x", "v", "f") else np.int32)
        self.scatter_atoms(name, 1 if arr.dtype == np.float64 else 0, arr.shape[1] if arr.ndim > 1 else 1,
                           arr.ctypes.data_as(C.c_void_p))

    def bond_set(self):
        """Set of (type, lo_tag, hi_tag) over all stored bonds."""
        nb, bt, ba = self.gather("num_bond"), self.gather("bond_type"), self.gather("bond_atom")
        out = set()
        for i in np.nonzero(nb)[0]:
            for m in range(nb[i]):
                a, b = int(i) + 1, int(ba[i, m])
                out.add((int(bt[i, m]), min(a, b), max(a, b)))
        return out

    def pair_rows(self, cid):
        """The rows of a local compute (compute property/local, compute pair/local) as a float64 array of shape
        (rows, columns), one column per attribute of the compute: for the pair kinds the contact list of the current state,
        ordered by (lower ID, higher ID).  Raises LammpsError when the compute cannot answer (no run yet, or the host copies
        have replaced the device state)."""
        rows = self.extract_compute(cid, LMP_STYLE_LOCAL, LMP_SIZE_ROWS)
        if rows is None:
            raise LammpsError("no local compute with ID " + cid)
        cols = self.extract_compute(cid, LMP_STYLE_LOCAL, LMP_SIZE_COLS)
        width = max(cols, 1)
        out = np.empty((rows, width))
        if rows:
            p = self.lib.lammps_extract_compute(self.lmp, cid.encode(), LMP_STYLE_LOCAL, LMP_TYPE_ARRAY if cols else LMP_TYPE_VECTOR)
            self._check()
            if cols:
                pp = C.cast(p, C.POINTER(C.POINTER(C.c_double)))
                # (the rows are one contiguous block: row pointers into it)
                out[:] = np.ctypeslib.as_array(pp[0], shape=(rows, cols))
            else:
                out[:, 0] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(rows,))
        return out

    def angle_set(self):
        """{(type, a1, a2, a3)} of the copies the CENTRAL atoms store (one per angle), ends ordered."""
        na, at = self.gather("num_angle"), self.gather("angle_type")
        a1, a2, a3 = self.gather("angle_atom1"), self.gather("angle_atom2"), self.gather("angle_atom3")
        if at.ndim == 1:
            at, a1, a2, a3 = (v.reshape(-1, 1) for v in (at, a1, a2, a3))
        out = set()
        for i in np.nonzero(na)[0]:
            for m in range(na[i]):
                if a2[i, m] == i + 1:
                    out.add((int(at[i, m]), int(min(a1[i, m], a3[i, m])), int(a2[i, m]), int(max(a1[i, m], a3[i, m]))))
        return out

    # -- ID-addressed access (python/lammps.py gather_atoms_subset / scatter_atoms_subset): only the requested rows travel --
    def gather_atoms_subset(self, name, type, count, ndata, ids):
        """As python/lammps.py: a ctypes array of ndata*count values in the order of `ids`."""
        cids = (C.c_int * ndata)(*[int(i) for i in ids[:ndata]])
        data = ((C.c_double if type == 1 else C.c_int) * (ndata * count))()
        self.lib.lammps_gather_atoms_subset(self.lmp, name.encode(), type, count, ndata, cids, data)
        self._check()
        return data

    def scatter_atoms_subset(self, name, type, count, ndata, ids, data):
        cids = (C.c_int * ndata)(*[int(i) for i in ids[:ndata]])
        self.lib.lammps_scatter_atoms_subset(self.lmp, name.encode(), type, count, ndata, cids, data)
        self._check()

    def gather_atoms_concat(self, name, type, count):
        """As python/lammps.py: every atom in the engine's local order (gather_atoms_concat("id", 0, 1) gives that order)."""
        n = self.get_natoms()
        data = ((C.c_double if type == 1 else C.c_int) * (n * count))()
        self.lib.lammps_gather_atoms_concat(self.lmp, name.encode(), type, count, data)
        self._check()
        return data

    def _shape(self, name):
        """(type, count) of a per-atom name, as gather() uses them."""
        if name in ("x", "v", "f"):
            return 1, 3
        if name in ("bond_type", "bond_atom"):
            return 0, self.extract_setting("bond_per_atom")
        if name == "special":
            return 0, self.extract_setting("maxspecial")
        if name in ("angle_type", "angle_atom1", "angle_atom2", "angle_atom3"):
            return 0, self.extract_setting("angle_per_atom")
        return 0, {"image": 3, "nspecial": 3}.get(name, 1)

    def gather_ids(self, name, ids):
        """numpy rows of `name` for the atom IDs `ids` (any order, repeats allowed): shape (len(ids), count), or
        (len(ids),) for one value per atom."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        type, count = self._shape(name)
        out = np.zeros((len(ids), count), dtype=np.float64 if type == 1 else np.int32)
        self.lib.lammps_gather_atoms_subset(self.lmp, name.encode(), type, count, len(ids),
                                            ids.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.c_void_p))
        self._check()
        return out[:, 0] if count == 1 else out

    def scatter_ids(self, name, ids, arr):
        """Set `name` of the atoms `ids` from the rows of `arr` (x v f: (K, 3); image: (K, 3) unpacked; type: (K,))."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        type = 1 if name in ("x", "v", "f") else 0
        arr = np.ascontiguousarray(arr, dtype=np.float64 if type == 1 else np.int32).reshape(len(ids), -1)
        self.lib.lammps_scatter_atoms_subset(self.lmp, name.encode(), type, arr.shape[1], len(ids),
                                             ids.ctypes.data_as(C.POINTER(C.c_int)), arr.ctypes.data_as(C.c_void_p))
        self._check()

    # -- computes and variables (python/lammps.py extract_compute / extract_variable / set_variable) --
    def extract_compute(self, cid, style, type):
        """style 0 global / 2 local; type 0 scalar, 1 vector, 2 array, 3 size vector, 4 rows, 5 cols (LMP_* constants).
        Returns a float, a list of floats, a list of rows, or an int; None where the compute has no such data."""
        p = self.lib.lammps_extract_compute(self.lmp, cid.encode(), style, type)
        self._check()
        if not p:
            return None
        if type in (3, 4, 5) or (style == 2 and type == 0):
            return C.cast(p, C.POINTER(C.c_int))[0]
        if type == 0:
            return C.cast(p, C.POINTER(C.c_double))[0]
        if style == 0:
            n = C.cast(self.lib.lammps_extract_compute(self.lmp, cid.encode(), style, 3), C.POINTER(C.c_int))[0]
            return list(C.cast(p, C.POINTER(C.c_double))[:n])
        rows = C.cast(self.lib.lammps_extract_compute(self.lmp, cid.encode(), 2, 4), C.POINTER(C.c_int))[0]
        if type == 1:
            return list(C.cast(p, C.POINTER(C.c_double))[:rows])
        cols = C.cast(self.lib.lammps_extract_compute(self.lmp, cid.encode(), 2, 5), C.POINTER(C.c_int))[0]
        pp = C.cast(p, C.POINTER(C.POINTER(C.c_double)))
        return [list(pp[r][:cols]) for r in range(rows)]

    def extract_variable(self, name, group=None, vartype=None):
        """equal-style: float; index / loop / string: str; unknown: None.  (The style comes from the engine, so `vartype`
        of python/lammps.py is accepted and not needed.)"""
        style = self.lib.lammps_extract_variable_datatype(self.lmp, name.encode())
        if style < 0:
            return None
        p = self.lib.lammps_extract_variable(self.lmp, name.encode(), group.encode() if group else None)
        self._check()
        if not p:
            return None
        if style == 0:
            val = C.cast(p, C.POINTER(C.c_double))[0]
            self.lib.lammps_free(p)
            return val
        return C.cast(p, C.c_char_p).value.decode()

    def set_variable(self, name, value):
        """Set a string-style variable; returns 0, or -1 if there is no string-style variable of that name."""
        r = self.lib.lammps_set_variable(self.lmp, name.encode(), str(value).encode())
        self._check()
        return r

    def has_id(self, category, name):
        return self.lib.lammps_has_id(self.lmp, category.encode(), name.encode()) != 0

    def id_count(self, category):
        return self.lib.lammps_id_count(self.lmp, category.encode())

    def available_ids(self, category):
        buf = C.create_string_buffer(256)
        out = []
        for i in range(self.id_count(category)):
            self.lib.lammps_id_name(self.lmp, category.encode(), i, buf, 256)
            out.append(buf.value.decode())
        return out

    def available_styles(self, category):
        buf = C.create_string_buffer(256)
        out = []
        for i in range(self.lib.lammps_style_count(self.lmp, category.encode())):
            self.lib.lammps_style_name(self.lmp, category.encode(), i, buf, 256)
            out.append(buf.value.decode())
        return out

    def force_timeout(self):
        self.lib.lammps_force_timeout(self.lmp)

    def has_style(self, category, name):
        return self.lib.lammps_has_style(self.lmp, category.encode(), name.encode()) != 0

    def stat(self, name):
        return self.lib.lammps_le_stat(self.lmp, name.encode())

    def minimize(self, etol, ftol, maxiter, maxeval):
        """`minimize etol ftol maxiter maxeval` (min_style cg | sd on the device) -> what the stats block prints: the stop
        criterion as text, iterations, force evaluations, the three energies, the final force norms and the last alpha."""
        self.command("minimize %.17g %.17g %d %d" % (etol, ftol, maxiter, maxeval))
        return dict(stop=MIN_STOP_STRINGS[int(self.stat("min_stop"))], iterations=int(self.stat("min_iterations")), evals=int(self.stat("min_evals")),
                    e_initial=self.stat("min_e_initial"), e_previous=self.stat("min_e_previous"), e_final=self.stat("min_e_final"),
                    fnorm=self.get_thermo("fnorm"), fmax=self.get_thermo("fmax"), alpha=self.stat("min_alpha"))

    def thermo_history(self):
        """Every thermo line printed so far: array of rows (step, temp, epair, emol, etotal, press, bonds)."""
        import numpy as np
        self.lib.lammps_le_thermo_log.restype = C.c_int
        self.lib.lammps_le_thermo_log.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        n = self.lib.lammps_le_thermo_log(self.lmp, None, 0)
        out = np.zeros((n, 7))
        if n:
            self.lib.lammps_le_thermo_log(self.lmp, out.ctypes.data_as(C.c_void_p), n)
        return out

    # -- ranks: one process per GPU, z-slab spatial decomposition (engine extension) --
    def comm_init(self, backend, rank, world, unique_id=b"", session="default"):
        """Join a group of `world` engine instances.  backend "rccl": unique_id = the 128-byte ncclUniqueId
        created on rank 0 by `comm_unique_id()` and broadcast by the launcher; backend "shm": file mailbox under
        /dev/shm (test transport, one process per rank); backend "local": the ranks are instances driven by threads
        of this process (development transport).  Must be called before the first run; every rank then issues the same commands."""
        self.lib.lammps_le_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
        buf = C.create_string_buffer(bytes(unique_id).ljust(128, b"\0"), 128)
        self.lib.lammps_le_comm_init(self.lmp, backend.encode(), rank, world, buf, session.encode())
        self._check()


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the launcher broadcasts it)."""
    lib = _load()
    buf = C.create_string_buffer(128)
    if lib.lammps_le_comm_unique_id(buf) != 0:
        raise LammpsError("could not create an RCCL unique id")
    return buf.raw


def use_torch_rccl():
    """Point the engine at the RCCL copy PyTorch has already loaded (torch/lib/librccl.so), so that the process runs one
    RCCL instance.  No effect when LAMMPS_LE_RCCL_LIB is set by the user or torch ships no copy."""
    if os.environ.get("LAMMPS_LE_RCCL_LIB"):
        return
    import torch
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    if os.path.exists(cand):
        os.environ["LAMMPS_LE_RCCL_LIB"] = cand


def init_from_torch_distributed(lmp):
    """Give every rank of an initialised torch.distributed group the same RCCL unique id and join the engine's
    own communicator (RANK / WORLD_SIZE from the process group).  Used by bench.py."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    if world == 1:
        return
    use_torch_rccl()
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.zeros(128, dtype=torch.uint8, device=dev)
    if rank == 0:
        t = torch.frombuffer(bytearray(comm_unique_id()), dtype=torch.uint8).to(dev)
    dist.broadcast(t, src=0)
    lmp.comm_init("rccl", rank, world, bytes(t.cpu().numpy().tobytes()))
