"""Which variant of the fused step kernel a time step takes (csrc/step_plan.h plan_step), without a device: the plan for
every request against the rules restated here, every fused plan against the instantiations the dispatcher of launch_step
holds (its own look-up through the test hook lammps_le_test_step_plan; nothing is launched), and the environment switches
re-read at every call."""
import ctypes
import itertools

import pytest

SIZES = (32000, 50000, 50001, 64000, 64001, 1000000)
# every switch of the step kernel off (the empty setting) / on, one at a time, plus the pairs the GPU suite runs with
KNOBS = [{}, {"LAMMPS_LE_LPB": "1"}, {"LAMMPS_LE_LPB": "4"}, {"LAMMPS_LE_LPB_MAX_N": "64000"}, {"LAMMPS_LE_LPB_MAX_N": "0"},
         {"LAMMPS_LE_AHEAD_MAX_N": "0"}, {"LAMMPS_LE_AHEAD_MAX_N": "1000000000"}, {"LAMMPS_LE_NO_FUSE": "1"},
         {"LAMMPS_LE_NO_FUSED_THERMO": "1"}, {"LAMMPS_LE_NO_FUSED_GROUPS": "1"}, {"LAMMPS_LE_NO_FUSED_BIN": "1"},
         {"LAMMPS_LE_STEP_LDS_PAD": "45000"}, {"LAMMPS_LE_DIAG_STEP": "2"},
         {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}, {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0", "LAMMPS_LE_DIAG_STEP": "8"},
         {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0", "LAMMPS_LE_NO_FUSED_THERMO": "1"}]
NAMES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
         "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_STEP_LDS_PAD", "LAMMPS_LE_DIAG_STEP")
UNFUSED = None


def _hook():
    from lammps_le_amd import library_path
    fn = ctypes.CDLL(library_path()).lammps_le_test_step_plan
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = None
    req, out = (ctypes.c_int * 11)(), (ctypes.c_int * 16)()

    def plan(n, dd, r):
        req[:] = r
        fn(n, dd, req, out)
        return list(out)
    return plan


def expected(n, dd, r, env):
    """The rules of the step kernel's choice: (the first ten flags of k_step's key in its bit order, bin, draws by the
    member-rank table, bits of the diagnostic pre-launch, LDS pad) or UNFUSED."""
    L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells = r
    L, N, I, P = bool(L), bool(N), bool(I), bool(P)
    if "LAMMPS_LE_NO_FUSE" in env:
        return UNFUSED
    lpb4 = int(env["LAMMPS_LE_LPB"]) == 4 if "LAMMPS_LE_LPB" in env else n <= int(env.get("LAMMPS_LE_LPB_MAX_N", 50000))
    ahead = n <= int(env.get("LAMMPS_LE_AHEAD_MAX_N", 64000))
    members = False
    if nvebit != 1 or lgbit != 1:
        if not P or "LAMMPS_LE_NO_FUSED_GROUPS" in env or (angles and ahead) or thermo:
            return UNFUSED
        variant = (L, N, False, True, 1, False, False, bool(angles), False, True)
        members = lgbit != 1
    elif thermo:
        if not P or dd or lpb4 or ahead or angles or "LAMMPS_LE_NO_FUSED_THERMO" in env or which >= 0:
            return UNFUSED
        variant = (L, False, I, True, 1, False, False, False, True, False)
        N = check = False        # (the energy variant is launched without the next step and without its displacement test)
    elif angles:
        if not P:
            return UNFUSED
        variant = (L, N, I, True, 1, False, ahead, True, False, False)
    elif lpb4:
        variant = (L, N, I, P, 4, False, True, False, False, False)
    else:
        variant = (L, N, I, P, 1, False, ahead, False, False, False)
    four = variant[4] == 4
    bins = bool(check and N and not dd and which < 0 and not four and "LAMMPS_LE_NO_FUSED_BIN" not in env and cells)
    diag = int(env.get("LAMMPS_LE_DIAG_STEP", 0))
    if not (L and r[1] and I and P and which < 0 and not four and not thermo):
        diag = 0
    return variant, bins, members, diag, int(env.get("LAMMPS_LE_STEP_LDS_PAD", 0))


def exists(L, N, I, P, LPB, DIAG, AHEAD, ANG, EF, GRP):
    """The rule of csrc/step_plan.h step_variant_exists, restated for the ten flags of the key a request without walls
    decides (LAZYV and WALL false): 77 of k_step's 105 instantiations - 16 * 3 + 8 * 2 + 4 + 8 + 1.  The other 28 are the
    four that take the velocities a rebuild left pending (tests/test_lazy_permute_cpu.py) and the 24 of fix wall/region
    (tests/test_wall_cpu.py)."""
    if DIAG:
        return (L, N, I, P, LPB, AHEAD, ANG, EF, GRP) == (True, True, True, True, 1, False, False, False, False)
    if GRP:
        return not I and P and LPB == 1 and not AHEAD and not EF
    if EF:
        return not N and P and LPB == 1 and not AHEAD and not ANG
    if ANG:
        return P and LPB == 1
    return LPB == 1 or AHEAD


def test_variant_count():
    combos = [c for c in itertools.product(*([(False, True)] * 4 + [(1, 4)] + [(False, True)] * 5)) if exists(*c)]
    assert len(combos) == 77


@pytest.mark.parametrize("env", KNOBS, ids=lambda e: "+".join("%s=%s" % (k[10:], v) for k, v in e.items()) or "defaults")
def test_plan_matches_rules_and_dispatcher(env, monkeypatch):
    for name in NAMES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = _hook()
    count = 0
    flags = list(itertools.product((0, 1), repeat=6))
    for n, dd, (nvebit, lgbit), which, check, cells in itertools.product(SIZES, (0, 1), ((1, 1), (2, 1), (1, 2), (2, 2), (2, 4)),
                                                                      (-1, 0, 1), (0, 1), (0, 1)):
        for L, N, I, P, angles, thermo in flags:
            r = (L, N, I, P, angles, thermo, nvebit, lgbit, which, check, cells)
            got, want = plan(n, dd, r), expected(n, dd, r, env)
            count += 1
            if want is UNFUSED:
                assert got[0] == 0, (n, dd, r, got)
                continue
            variant, bins, members, diag, pad = want
            assert got[0] == 1 and tuple(got[1:11]) == tuple(int(v) for v in variant), (n, dd, r, got, want)
            assert got[11:15] == [int(bins), int(members), diag, pad], (n, dd, r, got, want)
            assert exists(*variant) and got[15] == 1, (n, dd, r, got)       # a fused plan is one the dispatcher can launch
    assert count == 6 * 2 * 5 * 3 * 4 * 64


def test_all_variants_reachable_and_switches_reread(monkeypatch):
    """Every instantiation of the ten-argument subset (77) but the diagnostic one is some plan's answer; the switches are read at
    the call, not once per process."""
    plan = _hook()
    for name in NAMES:
        monkeypatch.delenv(name, raising=False)
    seen = set()
    for env in KNOBS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for n, (nvebit, lgbit), fl in itertools.product(SIZES, ((1, 1), (2, 2)), itertools.product((0, 1), repeat=6)):
            got = plan(n, 0, fl + (nvebit, lgbit, -1, 1, 1))
            if got[0]:
                seen.add(tuple(got[1:11]))
        for k in env:
            monkeypatch.delenv(k)
    assert len(seen) == 76 and all(exists(*(bool(v) if i != 4 else v for i, v in enumerate(s))) for s in seen)
    grouped = (1, 1, 1, 1, 0, 0, 2, 2, -1, 1, 1)
    assert plan(6000, 0, grouped)[0] == 1 and plan(6000, 0, grouped)[10] == 1
    monkeypatch.setenv("LAMMPS_LE_NO_FUSED_GROUPS", "1")
    assert plan(6000, 0, grouped)[0] == 0
    monkeypatch.delenv("LAMMPS_LE_NO_FUSED_GROUPS")
    assert plan(6000, 0, grouped)[0] == 1
    plain = (1, 1, 1, 1, 0, 0, 1, 1, -1, 1, 1)
    assert plan(6000, 0, plain)[5] == 4
    monkeypatch.setenv("LAMMPS_LE_LPB", "1")
    assert plan(6000, 0, plain)[5] == 1 and plan(6000, 0, plain)[11] == 1
    monkeypatch.setenv("LAMMPS_LE_NO_FUSE", "1")
    assert plan(6000, 0, plain)[0] == 0
