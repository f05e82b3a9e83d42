"""The phased k loop of the split contraction (SEEKR_GEMM_LOOP=1: four phases per k tile, the two wave rows one barrier
apart, LDS-DMA kept in flight across barriers under counted vmcnt; seekr_amd/csrc/gemm_phased_schedule.hpp) gives the bits
of the present loop.  The cases live in tools/gemm_loop_check.py, which switches the loop through the environment and
skr_ctx_reload_knobs inside one process of its own, as tools/epilogue_check.py does for the epilogue."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_loop_check.py"), *args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "gemm loop check ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_phased_loop_gives_the_present_loops_bits(precision):
    """uint32-identical results with SEEKR_GEMM_LOOP=1 and =0: self, plain, plain at an unaligned column offset, cross with
    mirror, row stripes (LOWER + SELF + PLAIN) and the fused edge list; 32, 64, 96, 160 and 256 columns (kt = 1, 2, 3, 5, 8:
    below, at and just past the prefetch depth), 1 024 and 16 384 (four k chunks), 512 columns in chunks of 1, 3 and 5 k
    tiles (5 + 5 + 5 + 1); rows 3 x 5, 1 500 x 1 111, 1 024 x 768 and 4 100 x 300 (more than 16 tiles along a side: the
    persistent instance).  bf16x3 reaches the split kernel from 1 024 columns on.  f16x3 plain blocks also against the
    oracle within 2e-6 + 1e-5 |r|."""
    _check("--precision", precision)


@pytest.mark.gpu
def test_phased_loop_repeats_its_own_bits():
    """Ten launches of the 4 100-row self-comparison per width and precision, each compared with the first: an LDS-DMA
    piece read before it landed would show as a tile that changes from launch to launch."""
    _check("--repeats")
