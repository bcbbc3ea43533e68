"""Which launches a reneighbor takes (csrc/rebuild_plan.h plan_rebuild), without a device: the plan for every combination of
facts against the rules restated in rebuild_rules.py, every plan with a build against the instantiations the build dispatcher
of rebuild_lists holds (its own look-up through the test hook lammps_le_test_rebuild_plan; nothing is launched), and the
environment switches re-read at every call of the hook.

The combinations: every fact that is a yes or no both ways; for the others the values at which a rule changes - bonds per
atom with the stride of their packed records (none; three: one int4; four: exclusions still from the bond-partner table,
two int4; five: neither), the special flags of every class a rule tells apart (none special; the 1-2 level dropped; two
levels dropped; the 1-2 level kept and another dropped; a fractional weight alone and beside a dropped level), tiled and
z-major rows, the first build of a run and a later one."""
import ctypes
import itertools

import numpy as np
import pytest

import rebuild_rules as R

KNOBS = [{}, {"LAMMPS_LE_BUILD_FP64": "1"}, {"LAMMPS_LE_DIAG_BUILD": "6"}, {"LAMMPS_LE_NO_DIRECT_RECV": "1"},
         {"LAMMPS_LE_TEST_OVERFLOW_AT": "1"}, {"LAMMPS_LE_FREEZE_IMAGES": "1"}]
BONDS = ((0, 4), (3, 4), (4, 8), (5, 8))                   # (bpa, bond_pack_stride)
SPECIAL = ((1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 0, 1), (2, 1, 1), (0, 1, 2))
YESNO = [k for k, name in enumerate(R.FACTS) if name not in ("bpa", "bond_pack_stride", "sf1", "sf2", "sf3", "row_tile", "builds")]


def all_facts():
    """Every combination, one row each: int32 [N, len(FACTS)]."""
    col = {name: k for k, name in enumerate(R.FACTS)}
    small = np.array([b + s + (t, n) for b, s, t, n in itertools.product(BONDS, SPECIAL, (0, 16), (0, 1))], dtype=np.int32)
    yn = ((np.arange(1 << len(YESNO))[:, None] >> np.arange(len(YESNO))) & 1).astype(np.int32)
    out = np.empty((len(yn), len(small), len(R.FACTS)), dtype=np.int32)
    out[:, :, YESNO] = yn[:, None, :]
    out[:, :, [col[n] for n in ("bpa", "bond_pack_stride", "sf1", "sf2", "sf3", "row_tile", "builds")]] = small[None, :, :]
    return out.reshape(-1, len(R.FACTS))


@pytest.fixture(scope="module")
def combos():
    f = all_facts()
    assert len(f) == (1 << 15) * 4 * 6 * 2 * 2
    return f


def ask(f):
    """The hook's answer for every row of f: int32 [N, 3]."""
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_rebuild_plan
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = None
    f = np.ascontiguousarray(f, dtype=np.int32)
    out = np.full((len(f), 3), -1, dtype=np.int32)
    a, b = f.ctypes.data, out.ctypes.data
    for pa, pb in zip(range(a, a + f.nbytes, f.strides[0]), range(b, b + out.nbytes, out.strides[0])):
        fn(pa, pb)
    return out


def exists(nosp, asym, frac):
    """k_build_neigh<NOSP, false, FRAC> without <true, ., true>, or k_build_neigh_asym<FRAC>."""
    return not (nosp and frac) and not (nosp and asym)


def build_of(bits):
    return bool(bits & R.NOSP), bool(bits & R.ASYM), bool(bits & R.FRAC)


@pytest.mark.parametrize("env", KNOBS, ids=lambda e: "+".join("%s=%s" % (k[10:], v) for k, v in e.items()) or "defaults")
def test_plan_matches_rules_and_dispatcher(env, combos, monkeypatch):
    for name in R.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = ask(combos)
    bits, diag = R.expected(combos.T, env)
    wrong = np.nonzero((got[:, 0] != bits) | (got[:, 1] != diag))[0]
    assert len(wrong) == 0, (dict(zip(R.FACTS, combos[wrong[0]])), hex(got[wrong[0], 0]), hex(bits[wrong[0]]))
    plans = got[:, 0]
    has = lambda b: (plans & b) != 0
    # every plan with a build names an instantiation that exists, and the dispatcher holds it; no other plan names one
    build = has(R.BUILD)
    assert np.array_equal(build, combos[:, R.FACTS.index("pair")] != 0)
    assert all(exists(*build_of(int(b))) for b in np.unique(plans[build] & (R.NOSP | R.ASYM | R.FRAC)))
    assert np.array_equal(got[:, 2] != 0, build)
    assert not (plans[~build] & (R.NOSP | R.ASYM | R.FRAC | R.EXCL_BPART | R.DDCODE | R.FP64 | R.DIAG_BUILD)).any()
    # every instantiation is some plan's answer
    assert {build_of(int(b)) for b in np.unique(plans[build])} == {c for c in itertools.product((False, True), repeat=3) if exists(*c)}
    # the step kernel's bins are used on one GPU only, and instead of k_wrap_bin
    dd = combos[:, R.FACTS.index("decomposed")] != 0
    assert not (has(R.PREBINNED) & (dd | has(R.WRAP_BIN))).any()
    assert not (dd & has(R.WRAP_BIN | R.PERMUTE_BONDS | R.CHECK_DEFERRED)).any() and not (~dd & has(R.MAP_FILL | R.DIRECT_RECV)).any()
    # the physical records move only where the permute writes the table from records of one int4
    phys = has(R.PERMUTE_PHYS)
    assert not (phys & ~(has(R.PERMUTE_BONDS) & (combos[:, R.FACTS.index("bond_pack_stride")] == 4))).any()
    assert not (has(R.BOND_PACK_PHYS) & ~phys).any() and np.array_equal(has(R.PERMUTE_BONDS), has(R.SORT_WRITES_MAP))
    # a table is written exactly once: by the permute or by k_bond_table; frozen images only by k_bond_table
    regrow = combos[:, R.FACTS.index("regrow")] != 0
    assert (has(R.PERMUTE_BONDS) ^ has(R.BOND_TABLE))[~regrow].all() and not (has(R.PERMUTE_BONDS) & has(R.FROZEN_IMAGES)).any()
    # a regrow pass: the bond table and the build (with the diagnostic build where that switch is set), nothing else
    want = R.BOND_TABLE | np.where(build, R.BUILD | (R.DIAG_BUILD if "LAMMPS_LE_DIAG_BUILD" in env else 0), 0)
    assert np.array_equal((plans & R.LAUNCHES)[regrow], want[regrow])


def test_scalar_rules_and_switches_reread(monkeypatch):
    """The rules for one vector of facts give what they give for arrays; the switches are read at the call, not once per process."""
    for name in R.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    plan = R.hook()
    chain = R.facts()
    bits = plan(chain)[0]
    assert plan(chain) == R.expected(chain, {}) + (1,)
    assert bits & R.LAUNCHES == R.WRAP_BIN | R.BOND_PACK_PHYS | R.SORT_WRITES_MAP | R.PERMUTE_BONDS | R.PERMUTE_PHYS | R.BUILD
    assert bits & ~R.LAUNCHES == R.EXCL_BPART          # k_build_neigh<false, false, false>, tiled rows
    slab = R.facts(decomposed=1, row_tile=0, map_stale=1, builds=1)
    changes = {"LAMMPS_LE_BUILD_FP64": ("1", chain, R.FP64), "LAMMPS_LE_DIAG_BUILD": ("6", chain, R.DIAG_BUILD),
               "LAMMPS_LE_NO_DIRECT_RECV": ("1", slab, R.DIRECT_RECV), "LAMMPS_LE_TEST_OVERFLOW_AT": ("1", slab, R.FORCE_OVERFLOW),
               "LAMMPS_LE_FREEZE_IMAGES": ("1", chain, R.FROZEN_IMAGES | R.BOND_TABLE | R.BOND_PACK_PHYS | R.SORT_WRITES_MAP |
                                           R.PERMUTE_BONDS | R.PERMUTE_PHYS)}
    assert set(changes) == set(R.SWITCHES)
    for name, (value, f, differ) in changes.items():
        before = plan(f)
        monkeypatch.setenv(name, value)
        during = plan(f)
        assert during == R.expected(f, {name: value}) + (1,)
        assert before[0] ^ during[0] == differ, name
        monkeypatch.delenv(name)
        assert plan(f) == before
    monkeypatch.setenv("LAMMPS_LE_DIAG_BUILD", "6")
    assert plan(chain)[1] == 7
