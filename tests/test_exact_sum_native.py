"""The device's exact-sum arithmetic, on the host: rag_fin_amd/csrc/exact_sum.h -- the decomposition of a value into
limb pieces and the carry-and-round routine that facet_stats.hip compiles for the GPU -- compiled with `g++
-fsanitize=address,undefined -fno-sanitize-recover=all` into a small driver (tests/native/exact_sum_main.cpp, the
sanitizer runtimes linked statically) and run as a child process.  Its result bits must equal
facets.stats_reference on the groups of tests/test_facet_stats_cpu.py, on random groups across 10^+-300, on groups
that put the sum's top bit at every one of the 66 limb boundaries +- 1 (reached directly, by a carry and by a
borrow, in both signs), and on rounding cases whose guard and sticky bits sit in different limbs.  A sanitizer
report aborts the child (non-zero exit)."""
import math
import os
import shutil
import struct
import subprocess

import pytest

from rag_fin_amd import facets
from test_facet_stats_cpu import GROUPS, random_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san") / "exact_sum_san"
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "rag_fin_amd", "csrc"), os.path.join(ROOT, "tests", "native", "exact_sum_main.cpp"),
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def run(driver, tmp_path, groups, is_f64=True):
    """The driver's compact records (8 int64 words each) of `groups`."""
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<q", len(groups)))
        for g in groups:
            f.write(struct.pack("<qq", 1 if is_f64 else 0, len(g)) + struct.pack(f"<{len(g)}{'d' if is_f64 else 'q'}", *g))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([driver, str(inp), str(outp)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stderr[-4000:]}"
    raw = open(outp, "rb").read()
    assert len(raw) == 64 * len(groups)
    return [struct.unpack_from("<8q", raw, 64 * i) for i in range(len(groups))]


def as_double(word: int) -> float:
    return struct.unpack("<d", struct.pack("<q", word))[0]


def check_f64(recs, groups):
    for rec, g in zip(recs, groups):
        want = facets.stats_reference(g, "f64")
        assert (rec[0], rec[1]) == (want["count"], want["nan"]), g
        if want["sum"] != want["sum"]:
            assert math.isnan(as_double(rec[2])), g
        else:
            assert rec[2] == struct.unpack("<q", struct.pack("<d", want["sum"]))[0], (g, as_double(rec[2]), want["sum"])
        if want["count"]:
            assert (as_double(rec[4]), as_double(rec[5])) == (want["min"], want["max"]), g


def boundary_groups():
    """The sum's top bit B (of the fixed-point image: the value is 2^(B - 1074) and up) at 32 j - 1, 32 j, 32 j + 1 for
    every limb j: alone with bits at guard and sticky, by a carry (x + x), by a borrow (2x - x), and negated."""
    out = []
    for j in range(66):
        for B in (32 * j - 1, 32 * j, 32 * j + 1):
            e = B - 1074
            if not -1074 <= e <= 1023:
                continue
            g = [math.ldexp(1.0, e)]
            if e - 54 >= -1074:
                g += [math.ldexp(1.0, e - 53), math.ldexp(1.0, e - 54)]
            out += [g, [-v for v in g]]
            if e - 1 >= -1074:
                out += [[math.ldexp(1.0, e - 1)] * 2, [-math.ldexp(1.0, e - 1)] * 2]
            if e + 1 <= 1023:
                out += [[math.ldexp(1.0, e + 1), -math.ldexp(1.0, e)], [-math.ldexp(1.0, e + 1), math.ldexp(1.0, e)]]
            if e + 1 <= 1023 and e - 52 >= -1074:   # 53 ones up to bit B, plus one ulp: the carry runs through them all
                ones = math.ldexp(2.0 - 2.0 ** -52, e)
                out += [[ones, math.ldexp(1.0, e - 52)], [-ones, -math.ldexp(1.0, e - 52)]]
    return out


def rounding_groups():
    """x = 2^e (even) or 2^e + ulp (odd) plus exactly half an ulp: a tie; a sticky bit 47 places below the guard -- always
    another limb -- breaks it upwards, the same bit subtracted borrows through the guard and breaks it downwards.  e
    steps through every position of the guard bit inside a limb."""
    out = []
    for e in list(range(-960, -960 + 64)) + list(range(0, 64)) + list(range(950, 1014)):
        half, far = math.ldexp(1.0, e - 53), math.ldexp(1.0, e - 100)
        for x in (math.ldexp(1.0, e), math.ldexp(1.0, e) + math.ldexp(1.0, e - 52)):
            out += [[x, half], [x, half, far], [x, half, -far], [-x, -half], [-x, -half, -far], [-x, -half, far],
                    [x, far], [x, -far]]
    return out


def test_the_groups_of_the_definition(driver, tmp_path):
    groups = list(GROUPS.values()) + random_groups(300, seed=7)
    check_f64(run(driver, tmp_path, groups), groups)
    rec = dict(zip(GROUPS, run(driver, tmp_path, list(GROUPS.values()))))
    assert rec["intermediate overflow"][2] == struct.unpack("<q", struct.pack("<d", 1e308))[0]
    assert rec["all -0.0"][2] == 0 and rec["empty"][:3] == (0, 0, 0) and math.isinf(as_double(rec["overflow"][2]))


def test_the_top_bit_at_every_limb_boundary(driver, tmp_path):
    groups = boundary_groups()
    assert len(groups) > 1000
    check_f64(run(driver, tmp_path, groups), groups)


def test_guard_and_sticky_in_different_limbs(driver, tmp_path):
    groups = rounding_groups()
    check_f64(run(driver, tmp_path, groups), groups)
    # the cases do round in both directions
    sums = [facets.stats_reference(g, "f64")["sum"] for g in groups[:8]]
    assert sums[0] != sums[1] and sums[0] == sums[2]


def test_int64_limbs(driver, tmp_path):
    groups = [[2 ** 63 - 1] * 5, [-2 ** 63] * 3, [], [0], [2 ** 53 + 1, -1, 7], [-1] * 9, [2 ** 32, -2 ** 32, 2 ** 31, -2 ** 31 - 1]]
    for rec, g in zip(run(driver, tmp_path, groups, is_f64=False), groups):
        want = facets.stats_reference(g, "i64")
        assert rec[0] == want["count"] and rec[1] == 0 and rec[2] + (rec[3] << 32) == want["sum"], g
        if g:
            assert (rec[4], rec[5]) == (want["min"], want["max"]), g
