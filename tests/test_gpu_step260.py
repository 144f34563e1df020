"""The 260 model's train step (3-D 260^3, batch 1, fp32 and bf16) held to the oracle: every convolution, transposed
convolution and kernel-gradient launch of the step on a thin slab, and the whole step once.

The tables list each distinct launch of EM2EM(260)'s compiled step with the step's own in-plane extents, channel split,
k / s / p and kernel layout, its views (skip crops, the cone windows of the cycle path, the negative-pad window of
g.bd.c0) and its epilogue (LeakyReLU, gate, skip-gradient add with offset, dropout frame and keep mode) -- rows of up to
256 voxels, planes of 65,536 under the magic divisions, the Winograd and stride-2 forms that only this size selects.
Only the depth is cut (fullsize_cases: `depth`), to 20 input planes: enough for two or more output planes beyond any
kernel's z-run, and the library still names the kernel symbol the full 260^3 geometry gets.  That equality is asserted
twice on the host, without a device: test_tables_cover_the_260_steps compares the rows' launches with the dry-built
step's (tests/test_step_admission.py) key by key, symbol included, and test_thin_rows_keep_the_cube_symbol asks the
library about each row at full depth too.  The thin slabs do not reach runs along the full depth; the whole-step test
and test_gpu_model260.py (the 260^3 forward) stand for those.

Each case runs through oracle/torch_ops.py (float64) on the same -- for bf16 tensors bf16-rounded -- operands under the
standing bars of fullsize_cases.py: 3e-5 (fp32 direct forms), 1e-5 (Winograd forms), 1e-5 and 3e-6 in L2 (fp32 kernel
gradients), 6e-3 (bf16 outputs), 2e-5 (bf16 kernel gradients); every bf16 convolution row also holds each stored element
to the rounded float64 reference (fullsize_cases.exact_checked, bf16_exact.py).  Outputs are windows of NaN-filled
tensors: a voxel left out fails the comparison, a plane written outside the window fails the guard check."""
import time

import numpy as np
import pytest
import torch

import fullsize_cases as F
from fullsize_cases import _b, _c

N, IS3D, EDGE = 1, True, 260
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from transfer_em_amd import hip_ops
    hip_ops.require_gpu()
    torch.set_num_threads(min(16, len(__import__("os").sched_getaffinity(0))))
    return hip_ops


@pytest.fixture(scope="module")
def T():
    from oracle import torch_ops
    return torch_ops


CONV_FP32 = [
    _c("g.c0", 'c1_mfma_k<8, false, 0>', 260, 1, 256, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1a", 'wino_conv_k<8, 8, 3, 0, 9>', 256, 8, 254, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1b", 'conv_direct_k<8, 0, 8, 0, false>', 254, 8, 126, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("g.d2a", 'wino_conv_k<8, 16, 2, 0, 9>', 126, 8, 124, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d2b", 'conv_s2_k<16, 1, 2, false>', 124, 16, 61, 16, 4, 2, 0, slope=0.3, depth=20),
    _c("g.u2a", 'wino_conv_k<16, 32, 2, 0, 17>', 61, 16, 59, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u2b", 'convT_mfma_k<32, 16, 12, 1, 1>', 59, 32, 118, 16, 4, 2, 1, T=True, slope=0.3, drop=(0, 118, 2), depth=20),
    _c("g.mid", 'wino_conv_k<32, 32, 2, 0, 9>', 118, 16, 116, 32, 3, 1, 0, ci1=16, in1=(124, 3), slope=0.3, depth=20),
    _c("g.u1a", 'wino_conv_k<32, 16, 2, 0, 9>', 116, 32, 114, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u1b", 'convT_mfma_k<16, 8, 12, 1, 1>', 114, 16, 228, 8, 4, 2, 1, T=True, slope=0.3, drop=(0, 228, 2), depth=20),
    _c("g.f1", 'wino_conv_k<16, 16, 2, 0, 9>', 228, 8, 226, 16, 3, 1, 0, ci1=8, in1=(254, 14), slope=0.3, depth=20),
    _c("g.f2", 'c1out_mfma_k<16, false, false>', 226, 16, 224, 1, 3, 1, 0, depth=20),
    _c("g.c0", 'c1_mfma_k<8, false, 0>', 224, 1, 232, 8, 3, 1, 6, slope=0.3, depth=20),
    _c("g.d1a", 'wino_conv_k<8, 8, 3, 0, 9>', 232, 8, 230, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1b", 'conv_s2_k<8, 1, 4, true>', 230, 8, 114, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("g.d2a", 'wino_conv_k<8, 16, 2, 0, 9>', 114, 8, 112, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d2b", 'conv_s2_k<16, 1, 2, false>', 112, 16, 55, 16, 4, 2, 0, slope=0.3, depth=20),
    _c("g.u2a", 'wino_conv_k<16, 32, 2, 0, 9>', 55, 16, 53, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u2b", 'convT_mfma_k<32, 16, 12, 1, 1>', 53, 32, 102, 16, 4, 2, 3, T=True, slope=0.3, drop=(8, 118, 2), depth=20),
    _c("g.mid", 'wino_conv_k<32, 32, 2, 0, 9>', 102, 16, 100, 32, 3, 1, 0, ci1=16, in1=(112, 5), slope=0.3, depth=20),
    _c("g.u1a", 'wino_conv_k<32, 16, 2, 0, 9>', 100, 32, 98, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u1b", 'convT_mfma_k<16, 8, 12, 1, 1>', 98, 16, 192, 8, 4, 2, 3, T=True, slope=0.3, drop=(18, 228, 2), depth=20),
    _c("g.f1", 'wino_conv_k<16, 16, 2, 0, 9>', 192, 8, 190, 16, 3, 1, 0, ci1=8, in1=(230, 20), slope=0.3, depth=20),
    _c("g.f2", 'c1out_mfma_k<16, false, false>', 190, 16, 188, 1, 3, 1, 0, depth=20),
    _c("d.d1a", 'c1_mfma_k<8, false, 0>', 224, 1, 222, 8, 3, 1, 0, in0=(260, 18), slope=0.3, depth=20),
    _c("d.d1b", 'conv_s2_k<8, 1, 4, true>', 222, 8, 110, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("d.hack", 'wino_conv_k<8, 16, 2, 0, 9>', 110, 8, 108, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d2a", 'wino_conv_k<16, 32, 2, 0, 9>', 108, 16, 106, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d2b", 'conv_s2_k<32, 1, 1, false>', 106, 32, 52, 32, 4, 2, 0, slope=0.3, depth=20),
    _c("d.d3a", 'wino_conv_k<32, 32, 2, 0, 9>', 52, 32, 50, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d3b", 'conv_s2_k<32, 1, 1, false>', 50, 32, 24, 32, 4, 2, 0, slope=0.09, depth=20),
    _c("d.d1a", 'c1_mfma_k<8, false, 0>', 224, 1, 222, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.bd.f2", 'c1_mfma_k<16, true, 1>', 224, 1, 226, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f1", 'wino_conv_k<16, 16, 2, 2, 9>', 226, 16, 228, 8, 3, 1, 2, co1=8, gate=0.3, drop=(0, 228, 2), layout=1, depth=20),
    _c("g.bd.u1b", 'conv_s2_k<8, 1, 2, false>', 228, 8, 114, 16, 4, 2, 1, gate=0.3, depth=20),
    _c("g.bd.u1a", 'wino_conv_k<16, 32, 2, 1, 17>', 114, 16, 116, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.mid", 'wino_conv_k<32, 32, 2, 2, 9>', 116, 32, 118, 16, 3, 1, 2, co1=16, gate=0.3, drop=(0, 118, 2), layout=1, depth=20),
    _c("g.bd.u2b", 'conv_s2_k<16, 2, 2, false>', 118, 16, 59, 32, 4, 2, 1, gate=0.3, depth=20),
    _c("g.bd.u2a", 'wino_conv_k<32, 16, 2, 1, 9>', 59, 32, 61, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d2b", 'convT_mfma_k<16, 16, 12, 1, 2>', 61, 16, 124, 16, 4, 2, 0, T=True, gate=0.3, add=(118, 3), depth=20),
    _c("g.bd.d2a", 'wino_conv_k<16, 8, 2, 1, 9>', 124, 16, 126, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d1b", 'convT_mfma_k<8, 8, 12, 1, 2>', 126, 8, 254, 8, 4, 2, 0, T=True, gate=0.3, add=(228, 14), depth=20),
    _c("g.bd.d1a", 'wino_conv_k<8, 8, 3, 1, 9>', 254, 8, 256, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f2", 'c1_mfma_k<16, true, 1>', 188, 1, 190, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f1", 'wino_conv_k<16, 16, 2, 2, 9>', 190, 16, 192, 8, 3, 1, 2, co1=8, gate=0.3, drop=(18, 228, 2), layout=1, depth=20),
    _c("g.bd.u1b", 'conv_s2_k<8, 1, 2, false>', 192, 8, 98, 16, 4, 2, 3, gate=0.3, depth=20),
    _c("g.bd.u1a", 'wino_conv_k<16, 32, 2, 1, 9>', 98, 16, 100, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.mid", 'wino_conv_k<32, 32, 2, 2, 9>', 100, 32, 102, 16, 3, 1, 2, co1=16, gate=0.3, drop=(8, 118, 2), layout=1, depth=20),
    _c("g.bd.u2b", 'conv_s2_k<16, 2, 2, false>', 102, 16, 53, 32, 4, 2, 3, gate=0.3, depth=20),
    _c("g.bd.u2a", 'wino_conv_k<32, 16, 2, 1, 9>', 53, 32, 55, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d2b", 'convT_mfma_k<16, 16, 12, 1, 2>', 55, 16, 112, 16, 4, 2, 0, T=True, gate=0.3, add=(102, 5), depth=20),
    _c("g.bd.d2a", 'wino_conv_k<16, 8, 2, 1, 17>', 112, 16, 114, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d1b", 'convT_mfma_k<8, 8, 12, 1, 2>', 114, 8, 230, 8, 4, 2, 0, T=True, gate=0.3, add=(192, 20), depth=20),
    _c("g.bd.d1a", 'wino_conv_k<8, 8, 3, 1, 9>', 230, 8, 232, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.c0", 'c1out_mfma_k<8, true, false>', 232, 8, 224, 1, 3, 1, -4, layout=1, depth=20),
    _c("d.bd.d3b", 'convT_mfma_k<32, 32, 12, 1, 2>', 24, 32, 50, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d3a", 'wino_conv_k<32, 32, 2, 1, 9>', 50, 32, 52, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.d2b", 'convT_mfma_k<32, 32, 12, 1, 2>', 52, 32, 106, 32, 4, 2, 0, T=True, gate=0.3, depth=20),
    _c("d.bd.d2a", 'wino_conv_k<32, 16, 2, 1, 9>', 106, 32, 108, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.hack", 'wino_conv_k<16, 8, 2, 1, 9>', 108, 16, 110, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.d1b", 'convT_mfma_k<8, 8, 12, 1, 2>', 110, 8, 222, 8, 4, 2, 0, T=True, gate=0.3, depth=20),
    _c("d.bd.d1a", 'c1out_mfma_k<8, true, false>', 222, 8, 224, 1, 3, 1, 2, layout=1, depth=20),
]
BWW_FP32 = [
    _b("g.bww.f2", 'bww_c1m_k<16>', 226, 16, 224, 1, 3, 1, 0, depth=20),
    _b("g.bww.f1", 'wino_bww_k<16, 16, 2, false, 9>', 228, 8, 226, 16, 3, 1, 0, ci1=8, in1=(254, 14), depth=20),
    _b("g.bww.u1b", 'bww_s2_k<8, 16, 4, 2>', 228, 8, 114, 16, 4, 2, 1, depth=20),
    _b("g.bww.u1a", 'wino_bww_k<32, 16, 2, false, 17>', 116, 32, 114, 16, 3, 1, 0, depth=20),
    _b("g.bww.mid", 'wino_bww_k<32, 32, 2, false, 17>', 118, 16, 116, 32, 3, 1, 0, ci1=16, in1=(124, 3), depth=20),
    _b("g.bww.u2b", 'bww_s2_k<16, 32, 4, 2>', 118, 16, 59, 32, 4, 2, 1, depth=20),
    _b("g.bww.u2a", 'wino_bww_k<16, 32, 2, false, 9>', 61, 16, 59, 32, 3, 1, 0, depth=20),
    _b("g.bww.d2b", 'bww_s2_k<16, 16, 4, 2>', 124, 16, 61, 16, 4, 2, 0, depth=20),
    _b("g.bww.d2a", 'wino_bww_k<8, 16, 2, false, 9>', 126, 8, 124, 16, 3, 1, 0, depth=20),
    _b("g.bww.d1b", 'bww_s2tb_k<8>', 254, 8, 126, 8, 4, 2, 0, depth=20),
    _b("g.bww.d1a", 'wino_bww_k<8, 8, 2, true, 9>', 256, 8, 254, 8, 3, 1, 0, depth=20),
    _b("g.bww.c0", 'bww_c1m_k<8>', 260, 1, 256, 8, 3, 1, 0, depth=20),
    _b("g.bww.f2", 'bww_c1m_k<16>', 190, 16, 188, 1, 3, 1, 0, depth=20),
    _b("g.bww.f1", 'wino_bww_k<16, 16, 2, false, 9>', 192, 8, 190, 16, 3, 1, 0, ci1=8, in1=(230, 20), depth=20),
    _b("g.bww.u1b", 'bww_s2_k<8, 16, 4, 2>', 192, 8, 98, 16, 4, 2, 3, depth=20),
    _b("g.bww.u1a", 'wino_bww_k<32, 16, 2, false, 17>', 100, 32, 98, 16, 3, 1, 0, depth=20),
    _b("g.bww.mid", 'wino_bww_k<32, 32, 2, false, 17>', 102, 16, 100, 32, 3, 1, 0, ci1=16, in1=(112, 5), depth=20),
    _b("g.bww.u2b", 'bww_s2_k<16, 32, 4, 2>', 102, 16, 53, 32, 4, 2, 3, depth=20),
    _b("g.bww.u2a", 'wino_bww_k<16, 32, 2, false, 17>', 55, 16, 53, 32, 3, 1, 0, depth=20),
    _b("g.bww.d2b", 'bww_s2_k<16, 16, 4, 2>', 112, 16, 55, 16, 4, 2, 0, depth=20),
    _b("g.bww.d2a", 'wino_bww_k<8, 16, 2, false, 9>', 114, 8, 112, 16, 3, 1, 0, depth=20),
    _b("g.bww.d1b", 'bww_s2tb_k<8>', 230, 8, 114, 8, 4, 2, 0, depth=20),
    _b("g.bww.d1a", 'wino_bww_k<8, 8, 2, true, 9>', 232, 8, 230, 8, 3, 1, 0, depth=20),
    _b("g.bww.c0", 'bww_c1m_k<8>', 224, 1, 232, 8, 3, 1, 6, depth=20),
    _b("d.bww.d3b", 'bww_s2_k<32, 32, 4, 2>', 50, 32, 24, 32, 4, 2, 0, depth=20),
    _b("d.bww.d3a", 'wino_bww_k<32, 32, 2, false, 9>', 52, 32, 50, 32, 3, 1, 0, depth=20),
    _b("d.bww.d2b", 'bww_s2_k<32, 32, 4, 2>', 106, 32, 52, 32, 4, 2, 0, depth=20),
    _b("d.bww.d2a", 'wino_bww_k<16, 32, 2, false, 9>', 108, 16, 106, 32, 3, 1, 0, depth=20),
    _b("d.bww.hack", 'wino_bww_k<8, 16, 2, false, 9>', 110, 8, 108, 16, 3, 1, 0, depth=20),
    _b("d.bww.d1b", 'bww_s2tb_k<8>', 222, 8, 110, 8, 4, 2, 0, depth=20),
    _b("d.bww.d1a", 'bww_c1m_k<8>', 224, 1, 222, 8, 3, 1, 0, in0=(260, 18), depth=20),
    _b("d.bww.d1a", 'bww_c1m_k<8>', 224, 1, 222, 8, 3, 1, 0, depth=20),
]
CONV_BF16 = [
    _c("g.c0", 'c1_mfma_h_k<8, false, 0>', 260, 1, 256, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 8>', 256, 8, 254, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 254, 8, 126, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("g.d2a", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 126, 8, 124, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d2b", 'conv3_bf16_k<16, 16, 4, 2, 4, false, 8>', 124, 16, 61, 16, 4, 2, 0, slope=0.3, depth=20),
    _c("g.u2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 61, 16, 59, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u2b", 'convT_bf16_k<32, 16, 12, 1, 1>', 59, 32, 118, 16, 4, 2, 1, T=True, slope=0.3, drop=(0, 118, 2), depth=20),
    _c("g.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 118, 16, 116, 32, 3, 1, 0, ci1=16, in1=(124, 3), slope=0.3, depth=20),
    _c("g.u1a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 8>', 116, 32, 114, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u1b", 'convT_bf16_k<16, 8, 12, 1, 1>', 114, 16, 228, 8, 4, 2, 1, T=True, slope=0.3, drop=(0, 228, 2), depth=20),
    _c("g.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 8>', 228, 8, 226, 16, 3, 1, 0, ci1=8, in1=(254, 14), slope=0.3, depth=20),
    _c("g.f2", 'c1out_h_k<16, false, false>', 226, 16, 224, 1, 3, 1, 0, depth=20),
    _c("g.c0", 'c1_mfma_h_k<8, false, 0>', 224, 1, 232, 8, 3, 1, 6, slope=0.3, depth=20),
    _c("g.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 8>', 232, 8, 230, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 230, 8, 114, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("g.d2a", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 114, 8, 112, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.d2b", 'conv3_bf16_k<16, 16, 4, 2, 4, false, 8>', 112, 16, 55, 16, 4, 2, 0, slope=0.3, depth=20),
    _c("g.u2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 55, 16, 53, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u2b", 'convT_bf16_k<32, 16, 12, 1, 1>', 53, 32, 102, 16, 4, 2, 3, T=True, slope=0.3, drop=(8, 118, 2), depth=20),
    _c("g.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 102, 16, 100, 32, 3, 1, 0, ci1=16, in1=(112, 5), slope=0.3, depth=20),
    _c("g.u1a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 8>', 100, 32, 98, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("g.u1b", 'convT_bf16_k<16, 8, 12, 1, 1>', 98, 16, 192, 8, 4, 2, 3, T=True, slope=0.3, drop=(18, 228, 2), depth=20),
    _c("g.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 8>', 192, 8, 190, 16, 3, 1, 0, ci1=8, in1=(230, 20), slope=0.3, depth=20),
    _c("g.f2", 'c1out_h_k<16, false, false>', 190, 16, 188, 1, 3, 1, 0, depth=20),
    _c("d.d1a", 'c1_mfma_h_k<8, false, 0>', 224, 1, 222, 8, 3, 1, 0, in0=(260, 18), slope=0.3, depth=20),
    _c("d.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 222, 8, 110, 8, 4, 2, 0, slope=0.3, depth=20),
    _c("d.hack", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 110, 8, 108, 16, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 108, 16, 106, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d2b", 'conv_bf16_k<32, 32, 4, 2, 12, false>', 106, 32, 52, 32, 4, 2, 0, slope=0.3, depth=20),
    _c("d.d3a", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 52, 32, 50, 32, 3, 1, 0, slope=0.3, depth=20),
    _c("d.d3b", 'conv_bf16_k<32, 32, 4, 2, 12, false>', 50, 32, 24, 32, 4, 2, 0, slope=0.09, depth=20),
    _c("d.p1", 'conv_bf16_k<32, 32, 1, 1, 12, true>', 24, 32, 24, 32, 1, 1, 0, slope=0.3),
    _c("d.p2", 'conv_bf16_k<32, 1, 1, 1, 12, true>', 24, 32, 24, 1, 1, 1, 0, bias=True),
    _c("d.d1a", 'c1_mfma_h_k<8, false, 0>', 224, 1, 222, 8, 3, 1, 0, slope=0.3, depth=20),
    _c("g.bd.f2", 'c1_mfma_h_k<16, true, 1>', 224, 1, 226, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 5>', 226, 16, 228, 8, 3, 1, 2, co1=8, gate=0.3, drop=(0, 228, 2), layout=1, depth=20),
    _c("g.bd.u1b", 'conv3_bf16_k<8, 16, 4, 2, 8, false, 1>', 228, 8, 114, 16, 4, 2, 1, gate=0.3, depth=20),
    _c("g.bd.u1a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 1>', 114, 16, 116, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 5>', 116, 32, 118, 16, 3, 1, 2, co1=16, gate=0.3, drop=(0, 118, 2), layout=1, depth=20),
    _c("g.bd.u2b", 'conv3_bf16_k<16, 32, 4, 2, 4, true, 1>', 118, 16, 59, 32, 4, 2, 1, gate=0.3, depth=20),
    _c("g.bd.u2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 59, 32, 61, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d2b", 'convT_bf16_k<16, 16, 12, 1, 2>', 61, 16, 124, 16, 4, 2, 0, T=True, gate=0.3, add=(118, 3), depth=20),
    _c("g.bd.d2a", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 124, 16, 126, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 126, 8, 254, 8, 4, 2, 0, T=True, gate=0.3, add=(228, 14), depth=20),
    _c("g.bd.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 1>', 254, 8, 256, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f2", 'c1_mfma_h_k<16, true, 1>', 188, 1, 190, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 5>', 190, 16, 192, 8, 3, 1, 2, co1=8, gate=0.3, drop=(18, 228, 2), layout=1, depth=20),
    _c("g.bd.u1b", 'conv3_bf16_k<8, 16, 4, 2, 8, false, 1>', 192, 8, 98, 16, 4, 2, 3, gate=0.3, depth=20),
    _c("g.bd.u1a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 1>', 98, 16, 100, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 5>', 100, 32, 102, 16, 3, 1, 2, co1=16, gate=0.3, drop=(8, 118, 2), layout=1, depth=20),
    _c("g.bd.u2b", 'conv3_bf16_k<16, 32, 4, 2, 4, true, 1>', 102, 16, 53, 32, 4, 2, 3, gate=0.3, depth=20),
    _c("g.bd.u2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 53, 32, 55, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d2b", 'convT_bf16_k<16, 16, 12, 1, 2>', 55, 16, 112, 16, 4, 2, 0, T=True, gate=0.3, add=(102, 5), depth=20),
    _c("g.bd.d2a", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 112, 16, 114, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 114, 8, 230, 8, 4, 2, 0, T=True, gate=0.3, add=(192, 20), depth=20),
    _c("g.bd.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 1>', 230, 8, 232, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("g.bd.c0", 'c1out_h_k<8, true, false>', 232, 8, 224, 1, 3, 1, -4, layout=1, depth=20),
    _c("d.bd.p2", 'conv_bf16_k<1, 32, 1, 1, 12, true>', 24, 1, 24, 32, 1, 1, 0, gate=0.3, layout=1),
    _c("d.bd.p1", 'conv_bf16_k<32, 32, 1, 1, 12, true>', 24, 32, 24, 32, 1, 1, 0, gate=0.09, layout=1),
    _c("d.bd.d3b", 'convT_bf16_k<32, 32, 12, 1, 2>', 24, 32, 50, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d3a", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 1>', 50, 32, 52, 32, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.d2b", 'convT_bf16_k<32, 32, 12, 1, 2>', 52, 32, 106, 32, 4, 2, 0, T=True, gate=0.3, depth=20),
    _c("d.bd.d2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 106, 32, 108, 16, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.hack", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 108, 16, 110, 8, 3, 1, 2, gate=0.3, layout=1, depth=20),
    _c("d.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 110, 8, 222, 8, 4, 2, 0, T=True, gate=0.3, depth=20),
    _c("d.bd.d1a", 'c1out_h_k<8, true, false>', 222, 8, 224, 1, 3, 1, 2, layout=1, depth=20),
]
BWW_BF16 = [
    _b("g.bww.f2", 'bww_c1m_h_k<16>', 226, 16, 224, 1, 3, 1, 0, depth=20),
    _b("g.bww.f1", 'bww_bf16_k<16, 16, 3, 1, 12, 4, 27>', 228, 8, 226, 16, 3, 1, 0, ci1=8, in1=(254, 14), depth=20),
    _b("g.bww.u1b", 'bww_bf16_k<8, 16, 4, 2, 12, 4, 32>', 228, 8, 114, 16, 4, 2, 1, depth=20),
    _b("g.bww.u1a", 'bww_bf16_k<32, 16, 3, 1, 12, 4, 54>', 116, 32, 114, 16, 3, 1, 0, depth=20),
    _b("g.bww.mid", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 118, 16, 116, 32, 3, 1, 0, ci1=16, in1=(124, 3), depth=20),
    _b("g.bww.u2b", 'bww_bf16_k<16, 32, 4, 2, 12, 4, 32>', 118, 16, 59, 32, 4, 2, 1, depth=20),
    _b("g.bww.u2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 61, 16, 59, 32, 3, 1, 0, depth=20),
    _b("g.bww.d2b", 'bww_bf16_k<16, 16, 4, 2, 12, 4, 64>', 124, 16, 61, 16, 4, 2, 0, depth=20),
    _b("g.bww.d2a", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 126, 8, 124, 16, 3, 1, 0, depth=20),
    _b("g.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 254, 8, 126, 8, 4, 2, 0, depth=20),
    _b("g.bww.d1a", 'bww_bf16_k<8, 8, 3, 1, 12, 4, 14>', 256, 8, 254, 8, 3, 1, 0, depth=20),
    _b("g.bww.c0", 'bww_c1m_h_k<8>', 260, 1, 256, 8, 3, 1, 0, depth=20),
    _b("g.bww.f2", 'bww_c1m_h_k<16>', 190, 16, 188, 1, 3, 1, 0, depth=20),
    _b("g.bww.f1", 'bww_bf16_k<16, 16, 3, 1, 12, 4, 27>', 192, 8, 190, 16, 3, 1, 0, ci1=8, in1=(230, 20), depth=20),
    _b("g.bww.u1b", 'bww_bf16_k<8, 16, 4, 2, 12, 4, 32>', 192, 8, 98, 16, 4, 2, 3, depth=20),
    _b("g.bww.u1a", 'bww_bf16_k<32, 16, 3, 1, 12, 4, 54>', 100, 32, 98, 16, 3, 1, 0, depth=20),
    _b("g.bww.mid", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 102, 16, 100, 32, 3, 1, 0, ci1=16, in1=(112, 5), depth=20),
    _b("g.bww.u2b", 'bww_bf16_k<16, 32, 4, 2, 12, 4, 32>', 102, 16, 53, 32, 4, 2, 3, depth=20),
    _b("g.bww.u2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 55, 16, 53, 32, 3, 1, 0, depth=20),
    _b("g.bww.d2b", 'bww_bf16_k<16, 16, 4, 2, 12, 4, 64>', 112, 16, 55, 16, 4, 2, 0, depth=20),
    _b("g.bww.d2a", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 114, 8, 112, 16, 3, 1, 0, depth=20),
    _b("g.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 230, 8, 114, 8, 4, 2, 0, depth=20),
    _b("g.bww.d1a", 'bww_bf16_k<8, 8, 3, 1, 12, 4, 14>', 232, 8, 230, 8, 3, 1, 0, depth=20),
    _b("g.bww.c0", 'bww_c1m_h_k<8>', 224, 1, 232, 8, 3, 1, 6, depth=20),
    _b("d.bww.p2", 'bww_bf16_k<1, 32, 1, 1, 12, 4, 1>', 24, 32, 24, 1, 1, 1, 0),
    _b("d.bww.p1", 'bww_bf16_k<32, 32, 1, 1, 12, 4, 2>', 24, 32, 24, 32, 1, 1, 0),
    _b("d.bww.d3b", 'bww_bf16_k<32, 32, 4, 2, 12, 4, 32>', 50, 32, 24, 32, 4, 2, 0, depth=20),
    _b("d.bww.d3a", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 52, 32, 50, 32, 3, 1, 0, depth=20),
    _b("d.bww.d2b", 'bww_bf16_k<32, 32, 4, 2, 12, 4, 32>', 106, 32, 52, 32, 4, 2, 0, depth=20),
    _b("d.bww.d2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 108, 16, 106, 32, 3, 1, 0, depth=20),
    _b("d.bww.hack", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 110, 8, 108, 16, 3, 1, 0, depth=20),
    _b("d.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 222, 8, 110, 8, 4, 2, 0, depth=20),
    _b("d.bww.d1a", 'bww_c1m_h_k<8>', 224, 1, 222, 8, 3, 1, 0, in0=(260, 18), depth=20),
    _b("d.bww.d1a", 'bww_c1m_h_k<8>', 224, 1, 222, 8, 3, 1, 0, depth=20),
]

TABLES = {"fp32": (CONV_FP32, BWW_FP32), "bf16": (CONV_BF16, BWW_BF16)}


def _ids(rows):
    return [f"{i}-{r['name']}" for i, r in enumerate(rows)]


@gpu
@pytest.mark.parametrize("case", CONV_FP32, ids=_ids(CONV_FP32))
def test_convolution_260_step_shapes_fp32(H, T, oracle_lib, case):
    F.check_conv(H, T, oracle_lib, case, N, IS3D, False, seed=case["n"] + case["co0"])


@gpu
@pytest.mark.parametrize("case", BWW_FP32, ids=_ids(BWW_FP32))
def test_kernel_gradient_260_step_shapes_fp32(H, T, case):
    F.check_bww(H, T, case, N, IS3D, False, seed=case["n"] + case["co"])


@gpu
@pytest.mark.parametrize("case", CONV_BF16, ids=_ids(CONV_BF16))
def test_convolution_260_step_shapes_bf16(H, T, oracle_lib, case):
    F.check_conv(H, T, oracle_lib, case, N, IS3D, True, seed=case["n"] + case["co0"])


@gpu
@pytest.mark.parametrize("case", BWW_BF16, ids=_ids(BWW_BF16))
def test_kernel_gradient_260_step_shapes_bf16(H, T, case):
    F.check_bww(H, T, case, N, IS3D, True, seed=case["n"] + case["co"])


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_a_planted_error_fails_its_row(H, T, oracle_lib, bf16):
    """One tap of g.d1a's kernel scaled by 1.05 on the device, the true kernel in the reference: the row must fail --
    on the max-norm bar and, for bf16 tensors, on the element-by-element check of the stores as well."""
    case = next(c for c in TABLES["bf16" if bf16 else "fp32"][0] if c["name"] == "g.d1a")
    figures = {}
    with pytest.raises(AssertionError, match="g.d1a"):
        F.check_conv(H, T, oracle_lib, case, N, IS3D, bf16, seed=1, plant=True, report=figures)
    assert not all(e < figures["tol"] for e in figures["errs"])
    if bf16:
        assert figures["exact"]["fails"] > 0.10 * figures["exact"]["total"], figures["exact"]


# ------------------------------------------------------------------------------------------------ host: the tables and the step
def _host_launches(precision, cube=False):
    from transfer_em_amd import hip_ops
    conv, bww = TABLES[precision]
    bf16 = precision == "bf16"
    full = lambda c: dict(c, depth=None) if cube else c
    return [F.build_conv(hip_ops, full(c), N, IS3D, bf16, device="cpu")[0] for c in conv] + \
           [F.build_bww(hip_ops, full(c), N, IS3D, bf16, device="cpu")[0] for c in bww]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tables_cover_the_260_steps(monkeypatch, precision):
    """Every convolution / kernel-gradient launch of the dry-built 260^3 step has a row with the same key -- entry point,
    kernel symbol, in-plane extents, channels, views, k / s / p, layout and epilogue (fullsize_cases.thin_key) -- and
    every row is a launch of the step."""
    from test_step_admission import dry_step
    launches = _host_launches(precision)
    keys = {F.thin_key(l) for l in launches}
    assert len(keys) == len(launches), "two rows describe the same launch"
    with dry_step(monkeypatch, EDGE, IS3D, precision) as step:
        F.assert_tables_cover(step, keys, key=F.thin_key)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_thin_rows_keep_the_cube_symbol(precision):
    """The library's dry query names the same kernel for a row's thin slab and for the same row at full depth."""
    thin, cube = _host_launches(precision), _host_launches(precision, cube=True)
    conv, bww = TABLES[precision]
    for row, a, b in zip(conv + bww, thin, cube):
        assert a.meta["kernel"] == b.meta["kernel"] == row["kernel"], (row["name"], a.meta["kernel"], b.meta["kernel"])


# ------------------------------------------------------------------------------------------------ the whole step
@gpu
def test_train_step_260_runs(tmp_path):
    """EM2EM(260) trains: two steps in fp32 and in bf16, each under the multi-stream and the single-stream schedule.
    Losses and parameters are finite, the two schedules are bit-identical within a precision (every kernel is
    deterministic: a difference is a missing stream dependency), and the bf16 losses are within 5e-3 of the fp32 ones
    (the bar of test_train_step_bf16_132_full_size).  Standardized uint8 inputs at half amplitude (clear of the pole of
    the cycle / identity terms) and variance-preserving weights.  Prints the step time and the peak device memory."""
    from oracle import graph
    from transfer_em_amd.cgan import EM2EM
    from test_gpu_step import _inputs, _load, _state
    from util import rel_err
    shape = (1, EDGE, EDGE, EDGE, 1)
    rx = torch.from_numpy(np.float32(0.5) * _inputs(shape, 1234))
    ry = torch.from_numpy(np.float32(0.5) * _inputs(shape, 5678))
    st = _state(graph, True, True)
    runs = {}
    for prec in ("fp32", "bf16"):
        for streams in (True, False):
            torch.cuda.reset_peak_memory_stats()
            model = EM2EM(EDGE, f"{prec}{int(streams)}", seed=42, checkpoint_root=str(tmp_path), precision=prec, two_streams=streams)
            _load(model, st)
            losses = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses.append(model.train_step(rx, ry).cpu().numpy())
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            losses = np.stack(losses)
            theta = torch.cat([net.params.theta for net in model._nets]).cpu().numpy()
            print(f"260^3 {prec} {'multi-stream' if streams else 'single-stream'}: second step {dt * 1e3:.1f} ms (with the input "
                  f"copy), peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, losses {losses[1]}")
            assert np.isfinite(losses).all() and np.isfinite(theta).all(), (prec, streams, losses)
            runs[prec, streams] = (losses, theta)
            del model
            torch.cuda.empty_cache()
    for prec in ("fp32", "bf16"):
        assert np.array_equal(runs[prec, True][0], runs[prec, False][0]), prec
        assert np.array_equal(runs[prec, True][1], runs[prec, False][1]), prec
    assert rel_err(runs["bf16", True][0], runs["fp32", True][0]) < 5e-3, (runs["bf16", True][0], runs["fp32", True][0])
