"""The plan bit RB_LAZY_V (csrc/rebuild_plan.h): a rebuild leaves the velocities in the old order for the step kernel that
follows.  Without a device: the rule restated here, held against the hook lammps_le_test_rebuild_plan_lazy (the 22 facts of
lammps_le_test_rebuild_plan and, behind them, lazy_v) over every combination of the facts the rule reads, with and without
the switch LAMMPS_LE_PERMUTE_ALL; every other bit of the plan, and the whole answer of the old hook, are what the rules of
rebuild_rules.py give - the new fact and the new switch change nothing else."""
import ctypes
import itertools

import numpy as np
import pytest

import rebuild_rules as R

LAZY_V = 1 << 26
SWITCH = "LAMMPS_LE_PERMUTE_ALL"
DEPENDS = ("lazy_v", "can_defer", "sort_due", "decomposed", "regrow")          # the facts the rule reads
# ... each of them over a few surroundings that exercise the other rules of the plan (rebuild_rules.facts: the FENE chain)
AROUND = [{}, dict(bins_ready=1, counts_dirty=1), dict(bonds_dirty=1, snapshot_due=1), dict(bond_minimg=0), dict(bpa=5, bond_pack_stride=8),
          dict(sf1=1, sf2=1, sf3=1), dict(angles=1), dict(pair=0), dict(row_tile=0, map_stale=1, builds=1)]


def rule(lazy_v, can_defer, sort_due, decomposed, regrow, env):
    """The velocities stay behind only where the step kernel that takes them is certain to come next, on the order this
    rebuild leaves: the engine says that kernel follows (lazy_v) in one launch it looks behind (can_defer), no Atom::sort
    re-ranks the beads, one GPU, not the second pass of a rebuild whose lists overflowed, and the switch is not set."""
    return bool(lazy_v and can_defer and not sort_due and not decomposed and not regrow and SWITCH not in env)


def lazy_hook():
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_rebuild_plan_lazy
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = None
    buf, out = (ctypes.c_int * (len(R.FACTS) + 1))(), (ctypes.c_int * 1)()

    def plan(f, lazy_v):
        buf[:] = tuple(f) + (int(lazy_v),)
        fn(buf, out)
        return out[0]
    return plan


@pytest.mark.parametrize("env", [{}, {SWITCH: "1"}, {SWITCH: "1", "LAMMPS_LE_TEST_OVERFLOW_AT": "1"}, {"LAMMPS_LE_FREEZE_IMAGES": "1"}],
                         ids=lambda e: "+".join(sorted(k[10:] for k in e)) or "defaults")
def test_lazy_bit_follows_its_rule_and_nothing_else_moves(env, monkeypatch):
    for name in R.SWITCHES + (SWITCH,):
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    old, new = R.hook(), lazy_hook()
    rules_env = {k: v for k, v in env.items() if k != SWITCH}          # (rebuild_rules.py knows the switches of the parent)
    seen = set()
    for around in AROUND:
        for values in itertools.product((0, 1), repeat=len(DEPENDS)):
            v = dict(zip(DEPENDS, values))
            f = R.facts(**dict(around, **{k: v[k] for k in DEPENDS if k != "lazy_v"}))
            bits = new(f, v["lazy_v"])
            want = rule(env=env, **v)
            assert bool(bits & LAZY_V) == want, (around, v, hex(bits))
            # the rest of the plan is what the rules give, and what the old hook - which has no such fact - still answers
            expected = R.expected(f, rules_env)
            assert (bits & ~LAZY_V) == expected[0], (around, v, hex(bits), hex(expected[0]))
            assert old(f)[:2] == expected
            seen.add(want)
    assert seen == ({False} if SWITCH in env else {False, True})


def test_old_hook_never_shows_the_bit():
    """lammps_le_test_rebuild_plan keeps its 22 facts: the new one is false there, whatever the others are."""
    plan = R.hook()
    yn = [k for k, name in enumerate(R.FACTS) if name in ("decomposed", "bins_ready", "can_defer", "sort_due", "regrow", "pair", "angles")]
    for values in itertools.product((0, 1), repeat=len(yn)):
        f = list(R.facts())
        for k, val in zip(yn, values):
            f[k] = val
        bits, diag, _ = plan(tuple(f))
        assert not bits & LAZY_V and (bits, diag) == R.expected(tuple(f), {})


def test_the_bit_is_free_and_outside_the_launch_mask():
    taken = R.LAUNCHES | R.FROZEN_IMAGES | R.NOSP | R.ASYM | R.FRAC | R.EXCL_BPART | R.DDCODE | R.FP64
    assert not taken & LAZY_V and taken < LAZY_V
    assert np.int32(LAZY_V) > 0          # the hooks hand the bits out as a C int
