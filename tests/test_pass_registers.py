"""The two-tick pass holds its register line: every plain form of k_move_tt<TWO> - with and without the compact road
record (CREC) and the road state words (RSW) - fits the vector registers of the wavefronts per SIMD it is built for
(TT_WAVES, csrc/tfx_move_tt.hpp) without a byte of scratch.  The pass is bound by the cars' trip through HBM and gains
with every wavefront in flight; a spill puts scratch traffic into its tile loop, and until the walk
addressed its rows as a wave-uniform base plus one 32-bit offset per lane the shipped kernel carried two such dwords."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_regs  # noqa: E402

VGPRS_PER_SIMD = 512   # gfx950: per lane, shared by the wavefronts of a SIMD
VGPR_GRANULE = 8


def configured_waves():
    src = open(os.path.join(ROOT, "traffic-env_amd", "csrc", "tfx_move_tt.hpp")).read()
    return int(re.search(r"^#define TT_WAVES (\d+)$", src, re.M).group(1))


def vgpr_bound(waves):
    return VGPRS_PER_SIMD // waves // VGPR_GRANULE * VGPR_GRANULE


def test_the_bound_follows_the_wavefronts_per_simd():
    assert [vgpr_bound(w) for w in (5, 6, 7, 8)] == [96, 80, 72, 64]
    assert configured_waves() in (6, 7)


def test_plain_two_tick_pass_fits_its_registers_without_scratch():
    if not os.path.exists(kernel_regs.LIB):
        pytest.skip("library not built")
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    bound = vgpr_bound(configured_waves())
    plain = [k for k in kernel_regs.kernel_table() if k["name"].startswith("void k_move_tt<true, false, false, false, ")]
    # CREC x RSW, of which RSW without CREC does not exist (k_move_tt's static_assert)
    assert sorted(k["name"].split("(")[0] for k in plain) == [
        "void k_move_tt<true, false, false, false, false, false>",
        "void k_move_tt<true, false, false, false, true, false>",
        "void k_move_tt<true, false, false, false, true, true>"]
    for k in plain:
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["scratch_"] == 0, (k["name"], k["scratch_"])
        assert k["vgpr"] <= bound, (k["name"], k["vgpr"], bound)
