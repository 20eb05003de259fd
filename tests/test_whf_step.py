"""CPU: the Wichmann-Hill generator stepped with its state in single precision (isg_whf_*, instruct_amd/csrc/isg_wh.h) is the integer
generator of random.c:19-47: every state steps to (a*s) % m, the single precision uniform has the integer form's bits, the exact uniform is
the integer form's, and the state the redo path re-derives for one copy of a pass is the state the pass reached.  The header is compiled
here as the emulations compile it (gcc, -ffp-contract=off); the device runs the same code (tests/test_gpu_whf.py)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
LIB = os.path.join(EMUL, "libwhf_emul.so")
SRCS = [os.path.join(EMUL, "whf_emul.c")] + [os.path.join(ROOT, "instruct_amd", "csrc", f) for f in ("isg_wh.h", "isg_math.h")]
SEEDS = ((13, 4, 1972), (1, 1, 1), (30268, 30306, 30322))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        subprocess.check_call(["gcc", "-O2", "-std=gnu99","-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", LIB, SRCS[0], "-lm"])
    l = C.CDLL(LIB)
    for f in (l.whf_step_exhaustive, l.whf_from_reduces, l.whf_walk, l.whf_rederive):
        f.restype = C.c_long
    l.whf_walk.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_long]
    l.whf_rederive.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint]
    return l


def test_every_state_steps_to_the_integer_generators_successor(lib):
    assert lib.whf_step_exhaustive(0) == 0


def test_states_up_to_2000_above_the_modulus_step_correctly_too(lib):
    # isg_lcg_fast's domain (a * s < 2^24)
    assert lib.whf_step_exhaustive(2000) == 0


def test_from_reduces_states_at_or_above_the_modulus(lib):
    assert lib.whf_from_reduces() == 0


@pytest.mark.parametrize("seeds", SEEDS)
def test_a_million_steps_keep_state_and_both_values_equal_to_the_integer_form(lib, seeds):
    assert lib.whf_walk(seeds[0], seeds[1], seeds[2], 1000000) == 0


def test_walk_from_unreduced_seeds(lib):
    assert lib.whf_walk(40000, 65535, 123456, 1000) == 0


@pytest.mark.parametrize("vmask", [0b1111, 0b1010, 0b0101, 0b1001, 0b0110, 0b1000, 0b0001, 0b0111])
def test_redo_rederives_the_state_the_pass_reached(lib, vmask):
    for seeds in SEEDS + ((77, 30000, 9),):
        assert lib.whf_rederive(seeds[0], seeds[1], seeds[2], vmask) == 0
