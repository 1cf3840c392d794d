"""The padded row pitch of the walk's pending-pair store in LDS (dqmc_amd/csrc/scan_layout.h), checked without a GPU.

tests/uw_bank_model.cpp is a stand-alone host program (its own main) that includes the layout header the kernels use and models the
byte addresses of the 64 lanes of the two pivot reads of an accepted flip (ds_read_b128: four groups of 16 lanes, bank = (a / 4) mod
64, one extra cycle per extra distinct address on a bank).  It is compiled and run once; the tests assert on the figures it prints.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """{name: int} printed by the bank model, built with the host compiler against the layout header"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("uw_pitch") / "uw_bank_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dqmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "uw_bank_model.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_pivot_reads_are_conflict_free_with_the_padded_pitch(model):
    """every n = 1 .. 256 (16, 64, 80, 144 and 256 among them), every k = 1 .. 32, every pivot site: pa and pb cost 4 LDS cycles each"""
    assert model["padded_cases"] == 32 * sum(range(1, 257))
    assert model["padded_min_cycles"] == 4 and model["padded_max_cycles"] == 4


def test_the_model_sees_the_conflict_of_the_unpadded_pitch(model):
    """pitch = n, n = 16, 32, .. 256: pa costs 4 min(16, k) and pb 4 max(1, k - 16) cycles for every k and site -- the model tells the
    two layouts apart"""
    assert model["plain_cases"] == 32 * sum(range(16, 257, 16))
    assert model["plain_mismatches"] == 0
    assert model["plain_max_cycles"] == 64


def test_other_accesses_of_the_pair_store_are_no_worse(model):
    """the flip's pair store (ds_write_b128, contiguous in j: the 8 cycles of its 8 lane groups), the rebase copy's read (4) and the solo
    flush's operand read (ds_read_b64: 2-way in either layout) cost under the padded pitch what they cost under pitch = n"""
    for name in ("store_cycles", "rebase_read_cycles", "solo_flush_read_cycles"):
        assert model["padded_" + name] <= model["plain_" + name], name
    assert model["padded_store_cycles"] == 8 and model["padded_rebase_read_cycles"] == 4


def test_pitch_and_lds_budget(model):
    """pitch >= n, = 1 (mod 16), less than 16 above n for every n <= 1024; the N = 256 layout (kd = 32, register walk) and the largest
    layout any n asks for stay within the dynamic LDS the kernels request"""
    assert model["pitch_violations"] == 0
    assert model["pitch_256"] == 257
    assert model["lds_bytes_256"] == 143504
    assert model["lds_bytes_256"] <= model["lds_limit"] and model["lds_bytes_max"] <= model["lds_limit"]
    assert model["lds_limit"] == 160 * 1024
