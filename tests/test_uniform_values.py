"""What DSB_UNI promises (desamba_amd/csrc/dsb_classify_dev.h: "all lanes that are here hold this value"), checked: a second build of
the 64-lane emulation (tests/emu/build_emu64_uni.sh, the same sources) in which every DSB_UNI hands its value to
tests/emu/emu_uni_check.cpp, which compares it across the lanes that pass the site in the same stretch between two cross-lane
operations.  On the GPU a DSB_UNI of a value that differs from lane to lane would silently take lane 0's; here it is a finding with
its source line and read.  The sets and limits are those of tests/test_device_emu64.py; results equal to the oracle's.  Runs without a GPU."""
import ctypes as C
import os

import pytest

from conftest import GOLDEN, ROOT

LIB64U = os.path.join(ROOT, "tests", "emu", "libdsbemu64_uni.so")


@pytest.fixture(scope="module")
def emu_uni(demo, built):
    import importlib
    import emu_lib
    old = os.environ.get("DSB_EMU_LIB")
    os.environ["DSB_EMU_LIB"] = LIB64U
    try:
        importlib.reload(emu_lib)
        e = emu_lib.Emu(demo["index"])
    finally:
        if old is None:
            os.environ.pop("DSB_EMU_LIB", None)
        else:
            os.environ["DSB_EMU_LIB"] = old
        importlib.reload(emu_lib)
    e.L.dsb_uni_report.argtypes = [C.c_char_p, C.c_size_t]; e.L.dsb_uni_report.restype = C.c_int
    e.L.dsb_uni_checked.restype = C.c_ulong
    e.L.dsb_uni_set_read.argtypes = [C.c_int]
    return e


def uni_report(e):
    buf = C.create_string_buffer(1 << 16)
    n = e.L.dsb_uni_report(buf, len(buf))
    return n, [l for l in buf.value.decode().split("\n") if l]


def test_checker_reports_a_lane_dependent_value(emu_uni):
    """the checker's own kernel: four sites, one of them (line 2) fed `lane & 1`; the uniform ones -- before a wave_sync, in a section
    three lanes run, after that section -- are not reported"""
    uni_report(emu_uni)
    emu_uni.L.dsb_uni_set_read(1234)
    emu_uni.L.dsb_uni_selftest()
    n, lines = uni_report(emu_uni)
    assert n == 1, lines
    assert "line 2 " in lines[0] and "read 1234" in lines[0], lines
    assert uni_report(emu_uni)[0] == 0


@pytest.mark.parametrize("name,limit", [("ont20k", 12), ("pb", 12), ("ngs150", 150), ("appc", None), ("wrapq", None), ("overhang", None), ("ont5k_e25", 20), ("ngs_e14", 80), ("manyanchors", 1)])
def test_synthetic(emu_uni, oracle, name, limit):
    import desamba_amd as D
    uni_report(emu_uni)
    before = emu_uni.L.dsb_uni_checked()
    hist = 0
    for i, (rname, seq, q) in enumerate(D.read_fastq(os.path.join(GOLDEN, "synth", name + ".fq"), limit)):
        emu_uni.L.dsb_uni_set_read(i)
        exp = oracle.classify(seq, hist)
        got = emu_uni.classify(seq, hist)
        assert got == exp, rname
        n, lines = uni_report(emu_uni)
        assert n == 0, (rname, lines)
        f = emu_uni.findings()
        assert not f, (rname, f)
        hist = max(hist, len(seq))
    assert emu_uni.L.dsb_uni_checked() > before          # (the build under test is the checking one)
