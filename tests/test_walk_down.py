"""The walk in three launches (wk_block_body, wk_compose2_body, wk_down_body; instruct_amd/csrc/isg_walk.h) under host emulation, next to the
five bodies it replaces: on two copies of the same state both routes leave the same maps, entries, offsets, WkState and list counters, byte
for byte -- over several segments and super-blocks, over re-walks with kept origins, and where a path fails among the super-block maps, among
a super-block's block maps, inside a block's rows, on an irregular or an uncertain byte, or before it starts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
LIB = os.path.join(EMUL, "libwalk_down_emul.so")
SRCS = [os.path.join(EMUL, "walk_down_emul.cpp")] + [os.path.join(ROOT, "instruct_amd", "csrc", f) for f in
                                                     ("isg_walk.h", "isg_walk_plan.h", "isg_sampler.h", "isg_wh.h", "isg_math.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
CASES = ["exact_3seg", "interval_rewalks_1seg", "interval_rewalks_segs", "trimmed_tight", "miss_top", "miss_blocks", "miss_rows", "irregular", "irregular_untrimmed",
         "uncertain_strict", "uncertain_strict_rows", "carried_failure", "leaves_strip", "short_last_block", "threads_64"]
DIFF, FAIL, NFAIL_BLOCK, SEGS, SUPS, BLOCKS, OFF_STRIP, LDS_DOWN, FUSED, PROBES, SUM_D, CLEAN_FAIL = range(12)


def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRCS[0]])
    l = C.CDLL(LIB)
    l.wd_case_name.restype = C.c_char_p
    return l


def test_the_case_list_is_the_emulations():
    l = lib()
    assert [l.wd_case_name(k).decode() for k in range(l.wd_ncases())] == CASES


@pytest.mark.parametrize("name", CASES)
def test_three_launches_leave_what_the_five_bodies_leave_byte_for_byte(name):
    l = lib()
    out = np.zeros(12, dtype=np.uint64)
    rc = l.wd_case(CASES.index(name), out.ctypes)
    o = [int(v) for v in out]
    print(name, dict(diff=o[DIFF], fail=o[FAIL], nfail_block=o[NFAIL_BLOCK], segments=o[SEGS], supers=o[SUPS], blocks=o[BLOCKS], off_strip=o[OFF_STRIP], lds_down=o[LDS_DOWN],
                     probes=o[PROBES], sum_d=o[SUM_D]))
    assert rc == 0
    assert o[DIFF] == 0, "the routes differ (bits: table, maps, ent_sup, ent_blk, T, WkState, counters, probes, untouched words): %#x" % o[DIFF]
    assert o[FUSED] == 1 and o[LDS_DOWN] <= 160 * 1024
    assert o[CLEAN_FAIL] == 0 or name == "trimmed_tight"   # the unpatched scenario the patches are placed by resolves
    # each case reaches what it is there for
    if name == "exact_3seg":
        assert o[FAIL] == 0 and o[SEGS] == 3 and o[SUPS] == 9 and o[BLOCKS] == 120
    elif name == "interval_rewalks_1seg":
        assert o[FAIL] == 0 and o[SEGS] == 1 and o[SUPS] == 3 and o[PROBES] > 0
    elif name == "interval_rewalks_segs":
        assert o[FAIL] == 0 and o[SEGS] == 4 and o[PROBES] > 0
    elif name in ("trimmed_tight", "miss_top", "irregular", "uncertain_strict"):
        assert o[FAIL] == 1 and o[NFAIL_BLOCK] == 0      # a missed window found among the maps: no block is walked
    elif name == "miss_blocks":
        assert o[FAIL] == 0 and 0 < o[SUM_D]             # the blocks behind the missing delta have no entry, the others are walked
    elif name == "miss_rows":
        assert o[FAIL] == 1 and o[NFAIL_BLOCK] == 8      # wk_trim_range names the byte outside the row's columns a missed window
    elif name == "irregular_untrimmed":
        assert o[FAIL] == 2 and o[NFAIL_BLOCK] == 21
    elif name == "uncertain_strict_rows":
        assert o[FAIL] == 4 and o[NFAIL_BLOCK] > 0
    elif name == "carried_failure":
        assert o[FAIL] == 9 and o[SEGS] == 3
    elif name == "leaves_strip":
        assert o[FAIL] == 0 and o[OFF_STRIP] > 0
    elif name == "short_last_block":
        assert o[FAIL] == 0 and o[BLOCKS] == 2
    elif name == "threads_64":
        assert o[FAIL] == 0 and o[SEGS] == 3


def test_a_plan_whose_way_down_does_not_fit_the_lds_takes_the_five_launches():
    """windows of +-12 x 3 sqrt(gammas) in one segment: the F2 maps fill most of the 144 KB the plan allows them, and wk_down's strip and
    descriptors on top pass 160 KB; the same run with windows of +-4 sqrt(gammas) fits"""
    l = lib()
    out = np.zeros(3, dtype=np.uint64)
    assert l.wd_plan_limit(60000, C.c_double(3.0), C.c_double(12.0), 60000, C.c_ulonglong(160 * 1024), out.ctypes) == 0
    print("lds_down %d, lds_top %d, three launches %d" % tuple(out))
    assert out[0] > 160 * 1024 and out[1] <= 144 * 1024 and out[2] == 0
    assert l.wd_plan_limit(60000, C.c_double(1.0), C.c_double(4.0), 12800, C.c_ulonglong(160 * 1024), out.ctypes) == 0
    assert out[0] <= 160 * 1024 and out[2] == 1
    assert l.wd_plan_limit(60000, C.c_double(1.0), C.c_double(4.0), 12800, C.c_ulonglong(int(out[0]) - 1), out.ctypes) == 0
    assert out[2] == 0


def test_stand_alone_build_passes_one_run_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a host program of its own (the same file with its main): the LDS of the new bodies is allocated exactly as large as the plan says, so
    a staged region overrun is a heap overflow the sanitizer reports"""
    exe = str(tmp_path / "walk_down_asan")
    subprocess.check_call(["g++", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DWD_MAIN"] + FLAGS + ["-o", exe, SRCS[0]])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "0 of %d cases differ" % len(CASES) in r.stdout
