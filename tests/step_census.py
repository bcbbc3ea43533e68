"""The launch census of the step kernel for the tests: the key of an instantiation (csrc/step_plan.h StepKeyBit - the template
argument of k_step<KEY> -, force_variant_key) restated in Python, the engine's test hooks around it, and LIVE - the keys Engine::iterate can launch,
from a model of the requests it makes swept through the planner (lammps_le_test_step_plan_indent; nothing is launched)."""
import ctypes
import functools
import itertools
import os

from test_step_plan_cpu import KNOBS, NAMES, SIZES

STEP, FORCE = 0, 1
# the fifteen flags of k_step<KEY> in the key's bit order (csrc/step_plan.h StepKeyBit; LPB: lanes per bead, 1 | 4, bit 4 set for 4)
FLAGS = ("L", "N", "I", "P", "LPB", "DIAG", "AHEAD", "ANG", "EF", "GRP", "LAZYV", "WALL", "SOFT", "EXT", "INDENT")
FORCE_FLAGS = ("E", "P", "NOBOND", "SOFT")


def key(L=0, N=0, I=0, P=0, LPB=1, DIAG=0, AHEAD=0, ANG=0, EF=0, GRP=0, LAZYV=0, WALL=0, SOFT=0, EXT=0, INDENT=0):
    assert LPB in (1, 4)
    bits = (L, N, I, P, LPB == 4, DIAG, AHEAD, ANG, EF, GRP, LAZYV, WALL, SOFT, EXT, INDENT)
    return sum(1 << b for b, v in enumerate(bits) if v)


def force_key(E=0, P=0, NOBOND=0, SOFT=0):
    return sum(1 << b for b, v in enumerate((E, P, NOBOND, SOFT)) if v)


def flags(k):
    """key -> the fifteen flags as a tuple of ints"""
    return tuple((4 if (k >> 4) & 1 else 1) if b == 4 else (k >> b) & 1 for b in range(15))


def name(k, kernel=STEP):
    """a key in words, for error messages"""
    if kernel == FORCE:
        return "k_force<%s>" % " ".join(n for b, n in enumerate(FORCE_FLAGS) if (k >> b) & 1)
    f = flags(k)
    return "k_step<%s>" % " ".join(("LPB4" if n == "LPB" else n) for n, v in zip(FLAGS, f) if v not in (0, 1) or (v == 1 and n != "LPB"))


def names(keys, kernel=STEP):
    return ", ".join("%d %s" % (k, name(k, kernel)) for k in sorted(keys))


@functools.lru_cache(maxsize=None)
def lib():
    from lammps_le_amd import library_path
    L = ctypes.CDLL(library_path())
    PI, PLL = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    L.lammps_le_test_step_census.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, PI, PLL]
    L.lammps_le_test_step_census.restype = ctypes.c_int
    L.lammps_le_test_step_census_reset.argtypes = [ctypes.c_void_p]
    L.lammps_le_test_step_census_reset.restype = None
    L.lammps_le_test_step_keys.argtypes = [ctypes.c_int, ctypes.c_int, PI]
    L.lammps_le_test_step_keys.restype = ctypes.c_int
    L.lammps_le_test_step_key_decode.argtypes = [ctypes.c_int, ctypes.c_int, PI]
    L.lammps_le_test_step_key_decode.restype = None
    L.lammps_le_test_step_key.argtypes = [ctypes.c_int, PI]
    L.lammps_le_test_step_key.restype = ctypes.c_int
    L.lammps_le_test_step_dispatch.argtypes = [ctypes.c_int]
    L.lammps_le_test_step_dispatch.restype = ctypes.c_int
    L.lammps_le_test_step_plan_indent.argtypes = [ctypes.c_int, ctypes.c_int, PI, PI]
    L.lammps_le_test_step_plan_indent.restype = None
    return L


def existing_keys(kernel=STEP):
    """The keys of the instantiations that exist, as the engine enumerates them (no device)."""
    cap = 1 << 15
    buf = (ctypes.c_int * cap)()
    n = lib().lammps_le_test_step_keys(kernel, cap, buf)
    assert n <= cap
    return list(buf[:n])


def dispatched(k):
    """1: the launcher's table holds k_step<k> (its own look-up; nothing is launched, no device)"""
    return lib().lammps_le_test_step_dispatch(k)


def engine_key(f, kernel=STEP):
    arr = (ctypes.c_int * len(f))(*[int(v) for v in f])
    return lib().lammps_le_test_step_key(kernel, arr)


def engine_flags(k, kernel=STEP):
    out = (ctypes.c_int * 15)()
    lib().lammps_le_test_step_key_decode(kernel, k, out)
    return tuple(out[:4 if kernel == FORCE else 15])


def census(lmp, kernel=STEP):
    """{key: launches} of a handle (lammps_le_amd.lammps) so far"""
    cap = 256
    keys, counts = (ctypes.c_int * cap)(), (ctypes.c_longlong * cap)()
    n = lib().lammps_le_test_step_census(lmp.lmp, kernel, cap, keys, counts)
    assert n <= cap
    return {keys[k]: counts[k] for k in range(n)}


def census_reset(lmp):
    lib().lammps_le_test_step_census_reset(lmp.lmp)


# ------------------------------------------------------------------------------------------------------------------
# LIVE: what Engine::iterate (csrc/engine.cpp) can ask of plan_step, and what launch_step then launches
# ------------------------------------------------------------------------------------------------------------------
def engine_requests(dd):
    """The fifteen-number requests (the layout of lammps_le_test_step_plan_indent) Engine::iterate can make of a run that is
    decomposed (dd) or not."""
    for L, N, I, P, angles, thermo in itertools.product((0, 1), repeat=6):
        # iterate: `rq.next = it + 1 < nsteps` is false on the last step of a run alone, and that step has `ntimestep == endstep`,
        # which sets eflag and with it `rq.thermo = eflag || ext_sums` (run: `endstep = ntimestep + nsteps`; `run upto` shortens
        # nsteps; the minimiser never calls launch_step): next or thermo
        if not (N or thermo):
            continue
        # iterate: `rq.nvebit = fusable ? nbits[0] : 1; rq.lgbit = lg ? lg->groupbit : 1` - any group bit for fix nve, for fix
        # langevin only where there is one.  (`rq.ident = d.ident_order` is passed as it is: with groups plan_step itself sets
        # `p.ident = false`, the rank table serves both orders)
        groups = [(1, 1), (2, 1)] + ([(1, 2), (2, 2), (2, 4)] if L else [])
        # iterate: `rq.which = -1` for every launch but the two of `if (d.dd && next && overlap)`, and `if (angles_active())
        # overlap = false`: a phase 0 | 1 only when decomposed, with a next step, without an angle style
        phases = [-1] + ([0, 1] if dd and N and not angles else [])
        # iterate: `rq.pair = pair_force(); rq.soft = pair_soft` with Engine::pair_force() = pair_lj || pair_soft: soft only with pair
        softs = [0, 1] if P else [0]
        # iterate: `rq.walls = walls_request(this); rq.indents = indents_request(this)` (0 none, 1 all on group all, 2 one on a
        # group) and `rq.ext = forceoptab.n > 0`, each on its own
        for (nvebit, lgbit), which, soft, walls, indents, ext in itertools.product(groups, phases, softs, (0, 1, 2), (0, 1, 2), (0, 1)):
            # (`rq.check`, `rq.cells` decide the plan's `bin` and `check`, run-time arguments of the launch, not the instantiation)
            yield [L, N, I, P, angles, thermo, nvebit, lgbit, which, 1, 1, walls, soft, ext, indents]


def launched_by(out):
    """The keys launch_step launches for one answer of lammps_le_test_step_plan_indent (its 23 numbers)."""
    if not out[0]:
        return set()           # iterate: `plan_now()` unfused -> compute_forces, no k_step
    assert out[15] == 1, out   # (the dispatcher holds what the plan names)
    args = dict(zip(FLAGS[:10], out[1:11]), WALL=out[16], SOFT=out[18], EXT=out[19], INDENT=out[21])
    got = {key(**args)}
    # launch_step_kernel: `lazy_v = d.v_pending && takes_pending_v(p, d.dd != 0)`; v_pending is raised by the rebuild iterate
    # asks for with `reneighbor(plan.fused && !plan.ef, sort_due, takes_pending_v(plan, d.dd != 0))` alone: LAZYV only where
    # takes_pending_v holds (out[17])
    if out[17]:
        got.add(key(LAZYV=1, **args))
    # launch_step: `if (p.diag_bits)` the instantiation L N I P DIAG (key 47) goes first; plan_step sets diag_bits
    # from StepKnobs::diag_step = LAMMPS_LE_DIAG_STEP alone
    if out[13]:
        got.add(key(L=1, N=1, I=1, P=1, DIAG=1))
    return got


@functools.lru_cache(maxsize=None)
def live_keys():
    """LIVE: the union of launched_by over the engine's requests, the sizes and the switch sets of test_step_plan_cpu.py."""
    saved = {k: os.environ.pop(k) for k in NAMES if k in os.environ}
    fn = lib().lammps_le_test_step_plan_indent
    out = (ctypes.c_int * 23)()
    requests = {dd: [(ctypes.c_int * 15)(*r) for r in engine_requests(dd)] for dd in (0, 1)}
    live, seen = set(), set()
    try:
        for env in KNOBS:
            os.environ.update(env)
            for dd in (0, 1):
                for n in SIZES:
                    for req in requests[dd]:
                        fn(n, dd, req, out)
                        answer = bytes(out)
                        if answer not in seen:
                            seen.add(answer)
                            got = launched_by(list(out))
                            assert "LAMMPS_LE_DIAG_STEP" in env or not any(flags(k)[5] for k in got)      # DIAG only under the switch
                            live |= got
            for k in env:
                del os.environ[k]
    finally:
        for k in NAMES:
            os.environ.pop(k, None)
        os.environ.update(saved)
    return frozenset(live)


if __name__ == "__main__":
    # python tests/step_census.py 1039 47 ...: the flags of the k_step<KEY> a kernel trace or a census file shows
    import sys
    for arg in sys.argv[1:]:
        print(names([int(arg)]))
