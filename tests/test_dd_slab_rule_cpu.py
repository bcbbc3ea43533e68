"""The width rule of the z-slab decomposition (csrc/device.h slab_rule) without a device, through the test hook
lammps_le_test_slab_rule: a slab may be as thin as ONE ghost cutoff (a bead is then in both send lists), as long as it holds
two pair shells and the ghost shells of a rank do not overlap around the period.  Everything the earlier rule
(w >= 2 * cutghost and w + 2 * cutghost <= Lz) accepted stays accepted."""
import ctypes

import pytest

OK, BELOW_GHOST, BELOW_PAIR, OVERLAP = 0, 1, 2, 3
CUTNEIGH = 1.52          # rc 1.12 + skin 0.4 of the recommended script


def _rule():
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_slab_rule
    fn.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_char_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(512)

    def rule(lz, world, cutneigh, comm):
        code = fn(lz, world, cutneigh, comm, buf, len(buf))
        return code, buf.value.decode()
    return rule


@pytest.mark.parametrize("lz,world", [(49.62, 8), (29.56, 4), (29.56, 5), (42.23, 5), (42.23, 6)])
def test_slabs_between_one_and_two_ghost_cutoffs_are_accepted(lz, world):
    comm = 6.2 if lz == 42.23 else 5.0
    w = lz / world
    assert comm <= w < 2 * comm                     # the ground the earlier rule refused
    assert _rule()(lz, world, CUTNEIGH, comm) == (OK, "")


def test_everything_the_two_cutoff_rule_accepted_stays_accepted():
    rule, seen = _rule(), 0
    for lz in (29.56, 42.23, 49.62, 105.6):
        for world in range(2, 13):
            for cutneigh, comm in ((1.52, 5.0), (1.52, 2.0), (1.52, 6.2), (1.52, 0.0), (2.9, 3.0)):
                cutghost, w = max(cutneigh, comm), lz / world
                if w >= 2.0 * cutghost and w + 2.0 * cutghost <= lz:
                    seen += 1
                    assert rule(lz, world, cutneigh, comm)[0] == OK, (lz, world, cutneigh, comm)
    assert seen > 60


def test_a_slab_below_one_ghost_cutoff_is_refused():
    code, msg = _rule()(29.56, 6, CUTNEIGH, 5.0)       # w = 4.93
    assert code == BELOW_GHOST
    assert "one ghost cutoff" in msg and "4.92" in msg and "5.0" in msg       # names w and the cutoff
    assert "two ghost" not in msg


def test_a_slab_below_two_pair_shells_is_refused():
    # comm cutoff 2.0 < 2 * 1.52: w = 2.5 holds a ghost shell but not two pair shells
    code, msg = _rule()(30.0, 12, CUTNEIGH, 2.0)
    assert code == BELOW_PAIR and "two pair shells" in msg
    # no comm_modify cutoff at all: the ghost cutoff is the neighbor cutoff
    code, msg = _rule()(30.0, 9, CUTNEIGH, 0.0)        # w = 3.33 >= 3.04
    assert code == OK
    code, msg = _rule()(30.0, 10, 1.6, 0.0)            # w = 3.0 < 3.2
    assert code == BELOW_PAIR and "two pair shells" in msg


def test_overlapping_ghost_shells_are_refused():
    code, msg = _rule()(29.56, 2, CUTNEIGH, 8.0)       # w = 14.78 >= 8.0, but 14.78 + 16 > 29.56
    assert code == OVERLAP and "overlap" in msg


@pytest.mark.parametrize("lz,comm", [(29.56, 7.5), (42.23, 11.0), (20.0, 5.01)])
def test_two_ranks_need_two_ghost_cutoffs(lz, comm):
    """With two ranks w + 2 * cutghost <= Lz IS w >= 2 * cutghost: thin slabs mean three or more ranks."""
    w = lz / 2
    assert comm <= w < 2 * comm
    code, msg = _rule()(lz, 2, CUTNEIGH, comm)
    assert code == OVERLAP and "overlap" in msg
    assert _rule()(lz, 2, CUTNEIGH, w / 2)[0] == OK


def test_the_rule_agrees_with_its_three_conditions_everywhere():
    rule = _rule()
    for lz in (29.56, 42.23, 49.62, 105.6):
        for world in range(2, 13):
            for cutneigh in (1.52, 2.9):
                for comm in (0.0, 2.0, 3.0, 5.0, 6.2, 8.0, 12.0):
                    w, cg = lz / world, max(cutneigh, comm)
                    want = BELOW_GHOST if w < cg else BELOW_PAIR if w < 2 * cutneigh else OVERLAP if w + 2 * cg > lz else OK
                    assert rule(lz, world, cutneigh, comm)[0] == want, (lz, world, cutneigh, comm)
