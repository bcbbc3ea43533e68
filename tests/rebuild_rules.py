"""The rules of a reneighbor's plan (csrc/rebuild_plan.h plan_rebuild) restated, and the test hook that asks the library:
shared by tests/test_rebuild_plan_cpu.py (every combination of facts) and the GPU suites (the plan a run executed,
lammps_le_stat("rebuild_plan"), against the hook's answer for the facts the case is meant to produce)."""
import ctypes

# RebuildBit
WRAP_BIN, COUNT_MEMSET, MAP_FILL, BOND_PACK, BOND_PACK_PHYS, SORT_WRITES_MAP, PERMUTE_BONDS, PREBINNED, PERMUTE_PHYS, BOND_TABLE, \
    FROZEN_IMAGES, BUILD, NOSP, ASYM, FRAC, EXCL_BPART = (1 << k for k in range(16))
DDCODE_SHIFT, DDCODE = 16, 3 << 16
FP64, DIAG_BUILD, DIRECT_RECV, ANGLE_LIST, TOPO_SNAPSHOT, CHECK_DEFERRED, FORCE_OVERFLOW, ATOM_SORT = (1 << k for k in range(18, 26))
# what a plan launches or skips, as opposed to how the bond table and the build it holds are made
LAUNCHES = (WRAP_BIN | COUNT_MEMSET | MAP_FILL | BOND_PACK | BOND_PACK_PHYS | SORT_WRITES_MAP | PERMUTE_BONDS | PREBINNED | PERMUTE_PHYS |
            BOND_TABLE | BUILD | DIAG_BUILD | DIRECT_RECV | ANGLE_LIST | TOPO_SNAPSHOT | CHECK_DEFERRED | FORCE_OVERFLOW | ATOM_SORT)

FACTS = ("decomposed", "bins_ready", "counts_dirty", "bonds_dirty", "phys_valid", "bond_minimg", "bpa", "bond_pack_stride", "bpart",
         "pair", "sf1", "sf2", "sf3", "special_asym", "row_tile", "angles", "snapshot_due", "map_stale", "sort_due", "can_defer",
         "regrow", "builds")
SWITCHES = ("LAMMPS_LE_BUILD_FP64", "LAMMPS_LE_DIAG_BUILD", "LAMMPS_LE_NO_DIRECT_RECV", "LAMMPS_LE_TEST_OVERFLOW_AT",
            "LAMMPS_LE_FREEZE_IMAGES")


def facts(**kw):
    """A facts vector: one GPU, clean flags, the FENE chain's topology (two bonds per bead, `special_bonds fene`), a pair
    style, tiled rows, nothing else going on - with the named facts replaced."""
    f = dict.fromkeys(FACTS, 0)
    f.update(bond_minimg=1, bpa=2, bond_pack_stride=4, bpart=1, pair=1, sf1=0, sf2=1, sf3=1, row_tile=16)
    assert set(kw) <= set(FACTS), kw
    f.update(kw)
    return tuple(int(f[k]) for k in FACTS)


def hook(lib=None):
    """plan(facts) -> (bits, diag_bits, the build dispatcher holds the instantiation) under the environment as it stands."""
    if lib is None:
        from lammps_le_amd import library_path
        lib = ctypes.CDLL(library_path())
    fn = lib.lammps_le_test_rebuild_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = None
    buf, out = (ctypes.c_int * len(FACTS))(), (ctypes.c_int * 3)()

    def plan(f):
        buf[:] = f
        fn(buf, out)
        return out[0], out[1], out[2]
    return plan


def expected(f, env):
    """(bits, diag_bits) by the rules.  f: a facts vector, or a sequence of equally long integer arrays, one per fact (the
    rules are written with & | * so that they hold for both); env: the rebuild's switches that are set."""
    (dd, bins_ready, counts_dirty, bonds_dirty, phys_valid, minimg, bpa, stride, bpart, pair, sf1, sf2, sf3, asym, row_tile, angles,
     snapshot, map_stale, sort_due, can_defer, regrow, builds) = f
    no = lambda v: v == 0
    yes = lambda v: v != 0
    first = no(regrow)          # not a regrow pass: everything in front of and behind the lists stage
    minimg = yes(minimg) & ("LAMMPS_LE_FREEZE_IMAGES" not in env)
    permute_bonds = no(dd) & minimg & (bpa > 0) & yes(bpart)
    phys = permute_bonds & (stride == 4)
    prebinned = yes(bins_ready) & no(dd)
    overflow = builds == int(env["LAMMPS_LE_TEST_OVERFLOW_AT"]) if int(env.get("LAMMPS_LE_TEST_OVERFLOW_AT", -1)) >= 0 else builds != builds
    nosp = (sf1 == 1) & (sf2 == 1) & (sf3 == 1)
    frac = (sf1 == 2) | (sf2 == 2) | (sf3 == 2)
    pair = yes(pair)
    bits = (FORCE_OVERFLOW * (first & overflow)
            | PREBINNED * (first & prebinned)
            | WRAP_BIN * (first & no(prebinned) & no(dd))          # (decomposed: the migration pass bins)
            | COUNT_MEMSET * (first & yes(counts_dirty) & no(prebinned))
            | MAP_FILL * (first & yes(dd) & yes(map_stale))
            | BOND_PACK * (first & yes(bonds_dirty))
            | BOND_PACK_PHYS * (first & phys & (yes(bonds_dirty) | no(phys_valid)))
            | (SORT_WRITES_MAP | PERMUTE_BONDS) * (first & permute_bonds)
            | PERMUTE_PHYS * (first & phys)
            | DIRECT_RECV * (first & yes(dd) & ("LAMMPS_LE_NO_DIRECT_RECV" not in env))
            | ATOM_SORT * (first & yes(sort_due))
            | ANGLE_LIST * (first & yes(angles))
            | TOPO_SNAPSHOT * (first & yes(snapshot))
            | CHECK_DEFERRED * (first & yes(can_defer) & no(sort_due) & no(dd))
            | BOND_TABLE * (yes(regrow) | no(permute_bonds))
            | FROZEN_IMAGES * no(minimg)
            | BUILD * pair
            | NOSP * (pair & nosp)
            | ASYM * (pair & no(nosp) & yes(asym))
            | FRAC * (pair & frac)
            | EXCL_BPART * (pair & (sf1 == 0) & (sf2 == 1) & (sf3 == 1) & (bpa >= 1) & (bpa <= 4) & no(asym))
            | (1 << DDCODE_SHIFT) * (pair & yes(dd))
            | (2 << DDCODE_SHIFT) * (pair & no(dd) & no(row_tile))
            | FP64 * (pair & ("LAMMPS_LE_BUILD_FP64" in env))
            | DIAG_BUILD * (pair & ("LAMMPS_LE_DIAG_BUILD" in env)))
    diag = (int(env.get("LAMMPS_LE_DIAG_BUILD", 0)) | 1) * (pair & ("LAMMPS_LE_DIAG_BUILD" in env))
    return bits, diag
