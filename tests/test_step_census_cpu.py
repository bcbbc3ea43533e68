"""The launch census of the step kernel without a device: the key of an instantiation (csrc/step_plan.h StepKeyBit,
force_variant_key through the engine's test hooks), the set of instantiations Engine::iterate can launch (LIVE) and the set it
cannot (DORMANT) against literal tables, and the closing condition on the GPU matrix: the rows of
test_gpu_step_census.CASES, taken together, name every live instantiation - over the table, not over what happened to run.

LIVE comes from a model of the requests Engine::iterate makes (step_census.engine_requests: each clause restates an engine
line) swept through the planner itself over the sizes and switch sets of test_step_plan_cpu.py.  The model agrees with a
reading of the engine: a plan without a next step is asked for on the last step of a run alone, that step is a thermo step,
and with `thermo` set plan_step fuses the energy variant alone - so every NEXT = false instantiation outside the energy
variant (24 base, 12 each of WALL, SOFT, EXT, INDENT, 8 ANG, 4 GRP: 84 of 177) exists and is never launched.  The GPU test
holds the model to the engine: no run there may launch a key outside LIVE."""
import itertools

import numpy as np
import pytest

import step_census as sc
import test_step_plan_cpu as tp

# the flags of k_step<KEY> in the key's bit order: L, N, I, P, LPB, DIAG, AHEAD, ANG, EF, GRP, LAZYV, WALL, SOFT, EXT, INDENT
LIVE = {
    # base: 24
    (0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    # ANG: 8
    (0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    # GRP: 4
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    (0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0),
    # EF: 4
    (0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0),
    # LAZYV: 4
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0),
    # DIAG: 1
    (1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    # WALL: 12
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    # SOFT: 12
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    # EXT: 12
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    # INDENT: 12
    (0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 1, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
}

DORMANT = {
    # base: 24
    (0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    # ANG: 8
    (0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    # GRP: 4
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0),
    # WALL: 12
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    (0, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0), (1, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0),
    # SOFT: 12
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    (0, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0),
    # EXT: 12
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    (0, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
    # INDENT: 12
    (0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 0, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
    (0, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1), (1, 0, 1, 1, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1),
}


# k_force<E, P, NOBOND, SOFT>: ten exist, eight can be launched.  Engine::compute_forces (setup, unfused steps, minimize) calls
# launch_force with parts = 3 and either E; Engine::respa_level_forces - the one caller that splits the parts - always with
# eflag = false.  NOBOND (the pair part alone) with E = 1 is never asked for
FORCE_LIVE = {(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 1, 0, 1), (1, 1, 0, 1), (0, 1, 1, 0), (0, 1, 1, 1)}
FORCE_DORMANT = {(1, 1, 1, 0), (1, 1, 1, 1)}


def test_key_function():
    """The key is a bijection on the 177 + 10 instantiations, decode and key are inverse to each other (the engine's and the
    restatement of step_census.py alike), the bit order is that of StepKeyBit: LPB = 4 bit 4, LAZYV bit 10, INDENT
    bit 14; the enumeration agrees with the rule of test_step_plan_cpu.exists on the ten-argument subset."""
    keys, fkeys = sc.existing_keys(sc.STEP), sc.existing_keys(sc.FORCE)
    assert len(keys) == len(set(keys)) == 177 and len(fkeys) == len(set(fkeys)) == 10
    assert keys == sorted(keys) and all(0 <= k < 1 << 15 for k in keys) and all(0 <= k < 16 for k in fkeys)
    tuples = set()
    for k in keys:
        f = sc.engine_flags(k)
        assert f == sc.flags(k) and sc.engine_key(f) == k == sc.key(*f), (k, f)
        assert f[4] in (1, 4) and all(v in (0, 1) for b, v in enumerate(f) if b != 4)
        tuples.add(f)
    assert len(tuples) == 177
    for k in fkeys:
        f = sc.engine_flags(k, sc.FORCE)
        assert sc.engine_key(f, sc.FORCE) == k == sc.force_key(*f)
        assert (f[1] or not f[2]) and (f[1] or not f[3])          # the condition of launch_force
    assert {sc.engine_flags(k, sc.FORCE) for k in fkeys} == FORCE_LIVE | FORCE_DORMANT
    assert sc.key(LPB=4) == 1 << 4 and sc.key(LAZYV=1) == 1 << 10 and sc.key(INDENT=1) == 1 << 14 and sc.key(L=1) == 1
    assert sc.engine_key((0, 0, 0, 0, 4) + (0,) * 10) == 16 and sc.engine_key((0,) * 4 + (1,) + (0,) * 5 + (1,) + (0,) * 4) == 1024
    ten = {f[:10] for f in tuples if not any(f[10:])}
    want = {c for c in itertools.product(*([(0, 1)] * 4 + [(1, 4)] + [(0, 1)] * 5)) if tp.exists(*(bool(v) if b != 4 else v for b, v in enumerate(c)))}
    assert ten == want and len(ten) == 77
    # a key that is no instantiation decodes, and is not enumerated
    assert sc.key(L=1, N=1, LAZYV=1, WALL=1) not in keys


def test_dispatch_table_holds_the_existing_keys():
    """The launcher's table (kernels_md.hip step_kernel, through lammps_le_test_step_dispatch: its own look-up, nothing is
    launched) holds a key of the whole key space exactly where the rule says the instantiation exists: 177 keys."""
    existing = set(sc.existing_keys())
    answers = [sc.dispatched(k) for k in range(1 << 15)]
    wrong = [k for k, held in enumerate(answers) if held != (1 if k in existing else 0)]
    assert not wrong, sc.names(wrong)
    assert sum(answers) == len(existing) == 177
    assert sc.dispatched(-1) == 0 and sc.dispatched(1 << 15) == 0


def test_live_and_dormant_tables():
    """LIVE and DORMANT as the model and the planner give them, against the tables above: a change to either set is an edit here."""
    live = {sc.flags(k) for k in sc.live_keys()}
    existing = {sc.flags(k) for k in sc.existing_keys()}
    assert live <= existing
    assert live == LIVE, (sorted(live - LIVE), sorted(LIVE - live))
    assert existing - live == DORMANT
    assert len(LIVE) == 93 and len(DORMANT) == 84 and not (LIVE & DORMANT) and LIVE | DORMANT == existing
    # the reading: dormant = no next step and not the energy variant, whatever else; live = the rest
    assert DORMANT == {f for f in existing if not f[1] and not f[8]}
    by_family = {}
    for f in DORMANT:
        fam = next((n for n, b in (("INDENT", 14), ("EXT", 13), ("SOFT", 12), ("WALL", 11), ("GRP", 9), ("ANG", 7)) if f[b]), "base")
        by_family[fam] = by_family.get(fam, 0) + 1
    assert by_family == dict(base=24, WALL=12, SOFT=12, EXT=12, INDENT=12, ANG=8, GRP=4)


def test_matrix_closes():
    """The closing condition: the union of the `expect` sets of the GPU matrix is LIVE for k_step and every launchable
    instantiation for k_force.  No exception list."""
    import test_gpu_step_census as gpu
    step = {sc.flags(k) for k in gpu.table_keys(sc.STEP)}
    assert step == LIVE, "not in any row: %s; in a row, not live: %s" % (sorted(LIVE - step), sorted(step - LIVE))
    force = {sc.engine_flags(k, sc.FORCE) for k in gpu.table_keys(sc.FORCE)}
    assert force == FORCE_LIVE, (sorted(FORCE_LIVE - force), sorted(force - FORCE_LIVE))
    # every row names keys that exist, with counts that are positive or left open
    for cid, c in gpu.CASES.items():
        assert set(c["step"]) <= set(sc.existing_keys()) and set(c["force"]) <= set(sc.existing_keys(sc.FORCE)), cid
        assert all(n is gpu.ANY or n > 0 for n in list(c["step"].values()) + list(c["force"].values())), cid
        assert c["step"] or c["force"], cid


@pytest.mark.parametrize("langevin", [0, 1])
@pytest.mark.parametrize("family", ["wall", "soft", "ext", "indent", "nopair"])
def test_inputs_of_the_new_rows(family, langevin):
    """The conditions on the runs of census_runs.py, from the references alone: the bead count separates the lane shapes
    (no multiple of 64, above 2048 - nine workgroups of one lane per bead, a count the launch grid pads -, under the 50000 up to
    which four lanes share a bead); beads within a cutoff of both faces of every periodic dimension; three or more list
    builds in the twelve steps, one of them on a plain step; the wall, the indenter, the tether and the pull act on beads at
    every evaluation with forces that show; the float64 restatement's deviation keeps every bound under its ceiling and no
    pair near a cutoff."""
    import census_runs as cr
    import force_compare as fc
    from systems import wrap_into_box
    s = cr.system()
    n = len(s["x"])
    assert n % 64 != 0 and 2048 < n < 50000 and (n + 255) // 256 >= 9
    x, _ = wrap_into_box(s)
    box = np.asarray(s["box"])
    for d in range(3):
        assert (x[:, d] - box[d, 0] < 1.12).sum() > 20 and (box[d, 1] - x[:, d] < 1.12).sum() > 20
    S, ref, dev, builds = cr.reference(family, langevin)
    assert len(builds) >= 3 and any(k % cr.THERMO for k in builds), builds
    for q, ceiling in fc.TRAJ_CEILING.items():
        fc.bound(dev[q], ceiling)
    if family != "nopair":
        assert float(min(ref["gaps"])) > cr.required_gap(S, dev)
    if family in ("wall", "indent", "ext"):
        assert len(ref["acting"]) == fc.STEPS + 1
        assert min(a[0] for a in ref["acting"]) >= 8 and min(a[1] for a in ref["acting"]) > 0.5, ref["acting"]
