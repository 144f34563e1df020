"""The 2-D train step of the reference's training example (132^2, batch 64) one launch at a time against the CPU oracle,
in both precisions: conv2d_bf16_k / convT2d_bf16_k / bww2d_bf16_k (and the 1x1 head on conv_bf16_k / bww_bf16_k) with
bf16 tensors, and the fp32 kernels the fp32 step launches on the same geometry -- that step is the yardstick of
test_train_step_bf16_2d_notebook_config.

CONV and BWW list every convolution, transposed-convolution and kernel-gradient launch of
EM2EM(132, is3d=False) at batch 64 once; a row names the kernel symbol (and the weight layout flag) per precision,
(bf16, fp32), None where that precision has no such launch (the fp32 discriminator head is one fused kernel).  At this
batch bww2d_bf16_k's workgroups own runs of several (image, band) units that cross image boundaries, and the blockIdx
decode of conv2d_bf16_k / convT2d_bf16_k sees grids 32 x larger than the batch-2 operator tests.
The coverage guards hold each table to its step.

Bars (fullsize_cases.py): bf16 outputs 6e-3, fp32 slabs from bf16 operands 2e-5 (test_gpu_bf16.py); fp32: 3e-5 for the
direct forms, 1e-5 (3e-6 in the L2 norm) for the kernel gradients (test_gpu_fullsize_oracle.py).  bf16 rows of at most
2^22 output elements also hold every stored element to the rounded float64 reference (fullsize_cases.exact_checked)."""
import pytest
import torch

import fullsize_cases as F
from fullsize_cases import _b, _c

pytestmark = pytest.mark.gpu
N, IS3D = 64, False


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


CONV = [
    _c("g.c0", ('conv2d_bf16_k<1, 8, 3, 1, 16>', 'conv_rows_k<1, 0, 8, 0, false, 3, 1, 4>'), 132, 1, 128, 8, 3, 1, 0, slope=0.3),
    _c("g.d1a", ('conv2d_bf16_k<8, 8, 3, 1, 16>', 'conv_rows_k<8, 0, 8, 0, false, 3, 1, 4>'), 128, 8, 126, 8, 3, 1, 0, slope=0.3),
    _c("g.d1b", ('conv2d_bf16_k<8, 8, 4, 2, 16>', 'conv_direct_k<8, 0, 8, 0, false>'), 126, 8, 62, 8, 4, 2, 0, slope=0.3),
    _c("g.d2a", ('conv2d_bf16_k<8, 16, 3, 1, 16>', 'conv_direct_k<8, 0, 16, 0, false>'), 62, 8, 60, 16, 3, 1, 0, slope=0.3),
    _c("g.d2b", ('conv2d_bf16_k<16, 16, 4, 2, 16>', 'conv_direct_k<16, 0, 16, 0, false>'), 60, 16, 29, 16, 4, 2, 0, slope=0.3),
    _c("g.u2a", ('conv2d_bf16_k<16, 32, 3, 1, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 29, 16, 27, 32, 3, 1, 0, slope=0.3),
    _c("g.u2b", ('convT2d_bf16_k<32, 16, 12, 0>', 'convT_direct_k<32, 16, 0, 16>'), 27, 32, 54, 16, 4, 2, 1, T=True, slope=0.3, drop=(0, 54, 1)),
    _c("g.mid", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<16, 16, 32, 0, false>'), 54, 16, 52, 32, 3, 1, 0, ci1=16, in1=(60, 3), slope=0.3),
    _c("g.u1a", ('conv2d_bf16_k<32, 16, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 0, false>'), 52, 32, 50, 16, 3, 1, 0, slope=0.3),
    _c("g.u1b", ('convT2d_bf16_k<16, 8, 12, 0>', 'convT_direct_k<16, 8, 0, 8>'), 50, 16, 100, 8, 4, 2, 1, T=True, slope=0.3, drop=(0, 100, 1)),
    _c("g.f1", ('conv2d_bf16_k<16, 16, 3, 1, 16>', 'conv_direct_k<8, 8, 16, 0, false>'), 100, 8, 98, 16, 3, 1, 0, ci1=8, in1=(126, 14), slope=0.3),
    _c("g.f2", ('conv2d_bf16_k<16, 1, 3, 1, 16>', 'conv_rows_k<16, 0, 1, 0, false, 3, 1, 4>'), 98, 16, 96, 1, 3, 1, 0),
    _c("g.c0", ('conv2d_bf16_k<1, 8, 3, 1, 16>', 'conv_rows_k<1, 0, 8, 0, false, 3, 1, 4>'), 96, 1, 104, 8, 3, 1, 6, slope=0.3),
    _c("g.d1a", ('conv2d_bf16_k<8, 8, 3, 1, 16>', 'conv_rows_k<8, 0, 8, 0, false, 3, 1, 4>'), 104, 8, 102, 8, 3, 1, 0, slope=0.3),
    _c("g.d1b", ('conv2d_bf16_k<8, 8, 4, 2, 16>', 'conv_direct_k<8, 0, 8, 0, false>'), 102, 8, 50, 8, 4, 2, 0, slope=0.3),
    _c("g.d2a", ('conv2d_bf16_k<8, 16, 3, 1, 16>', 'conv_direct_k<8, 0, 16, 0, false>'), 50, 8, 48, 16, 3, 1, 0, slope=0.3),
    _c("g.d2b", ('conv2d_bf16_k<16, 16, 4, 2, 16>', 'conv_direct_k<16, 0, 16, 0, false>'), 48, 16, 23, 16, 4, 2, 0, slope=0.3),
    _c("g.u2a", ('conv2d_bf16_k<16, 32, 3, 1, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 23, 16, 21, 32, 3, 1, 0, slope=0.3),
    _c("g.u2b", ('convT2d_bf16_k<32, 16, 12, 0>', 'convT_direct_k<32, 16, 0, 16>'), 21, 32, 38, 16, 4, 2, 3, T=True, slope=0.3, drop=(8, 54, 1)),
    _c("g.mid", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<16, 16, 32, 0, false>'), 38, 16, 36, 32, 3, 1, 0, ci1=16, in1=(48, 5), slope=0.3),
    _c("g.u1a", ('conv2d_bf16_k<32, 16, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 0, false>'), 36, 32, 34, 16, 3, 1, 0, slope=0.3),
    _c("g.u1b", ('convT2d_bf16_k<16, 8, 12, 0>', 'convT_direct_k<16, 8, 0, 8>'), 34, 16, 64, 8, 4, 2, 3, T=True, slope=0.3, drop=(18, 100, 1)),
    _c("g.f1", ('conv2d_bf16_k<16, 16, 3, 1, 16>', 'conv_direct_k<8, 8, 16, 0, false>'), 64, 8, 62, 16, 3, 1, 0, ci1=8, in1=(102, 20), slope=0.3),
    _c("g.f2", ('conv2d_bf16_k<16, 1, 3, 1, 16>', 'conv_rows_k<16, 0, 1, 0, false, 3, 1, 4>'), 62, 16, 60, 1, 3, 1, 0),
    _c("d.hack", ('conv2d_bf16_k<1, 16, 3, 1, 16>', 'conv_direct_k<1, 0, 16, 0, false>'), 96, 1, 94, 16, 3, 1, 0, in0=(132, 18), slope=0.3),
    _c("d.d2a", ('conv2d_bf16_k<16, 32, 3, 1, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 94, 16, 92, 32, 3, 1, 0, slope=0.3),
    _c("d.d2b", ('conv2d_bf16_k<32, 32, 4, 2, 16>', 'conv_direct_k<32, 0, 32, 0, false>'), 92, 32, 45, 32, 4, 2, 0, slope=0.3),
    _c("d.d3a", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<32, 0, 32, 0, false>'), 45, 32, 43, 32, 3, 1, 0, slope=0.3),
    _c("d.d3b", ('conv2d_bf16_k<32, 32, 4, 2, 16>', 'conv_direct_k<32, 0, 32, 0, false>'), 43, 32, 20, 32, 4, 2, 0, slope=0.09),
    _c("d.p1", ('conv_bf16_k<32, 32, 1, 1, 12, true>', None), 20, 32, 20, 32, 1, 1, 0, slope=0.3),
    _c("d.p2", ('conv_bf16_k<32, 1, 1, 1, 12, true>', None), 20, 32, 20, 1, 1, 1, 0, bias=True),
    _c("d.hack", ('conv2d_bf16_k<1, 16, 3, 1, 16>', 'conv_direct_k<1, 0, 16, 0, false>'), 96, 1, 94, 16, 3, 1, 0, slope=0.3),
    _c("g.bd.f2", ('conv2d_bf16_k<1, 16, 3, 1, 16>', 'conv_rows_k<1, 0, 16, 0, true, 3, 1, 4>'), 96, 1, 98, 16, 3, 1, 2, gate=0.3, layout=(1, 1)),
    _c("g.bd.f1", ('conv2d_bf16_k<16, 16, 3, 1, 16>', 'conv_direct_k<16, 0, 8, 8, false>'), 98, 16, 100, 8, 3, 1, 2, co1=8, gate=0.3, drop=(0, 100, 2), layout=(1, 0)),
    _c("g.bd.u1b", ('conv2d_bf16_k<8, 16, 4, 2, 16>', 'conv_direct_k<8, 0, 16, 0, false>'), 100, 8, 50, 16, 4, 2, 1, gate=0.3),
    _c("g.bd.u1a", ('conv2d_bf16_k<16, 32, 3, 1, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 50, 16, 52, 32, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.mid", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 16, false>'), 52, 32, 54, 16, 3, 1, 2, co1=16, gate=0.3, drop=(0, 54, 2), layout=(1, 0)),
    _c("g.bd.u2b", ('conv2d_bf16_k<16, 32, 4, 2, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 54, 16, 27, 32, 4, 2, 1, gate=0.3),
    _c("g.bd.u2a", ('conv2d_bf16_k<32, 16, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 0, false>'), 27, 32, 29, 16, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.d2b", ('convT2d_bf16_k<16, 16, 12, 2>', 'convT_direct_k<16, 16, 0, 16>'), 29, 16, 60, 16, 4, 2, 0, T=True, gate=0.3, add=(54, 3)),
    _c("g.bd.d2a", ('conv2d_bf16_k<16, 8, 3, 1, 16>', 'conv_direct_k<16, 0, 8, 0, false>'), 60, 16, 62, 8, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.d1b", ('convT2d_bf16_k<8, 8, 12, 2>', 'convT_direct_k<8, 8, 0, 8>'), 62, 8, 126, 8, 4, 2, 0, T=True, gate=0.3, add=(100, 14)),
    _c("g.bd.d1a", ('conv2d_bf16_k<8, 8, 3, 1, 16>', 'conv_direct_k<8, 0, 8, 0, true>'), 126, 8, 128, 8, 3, 1, 2, gate=0.3, layout=(1, 1)),
    _c("g.bd.f2", ('conv2d_bf16_k<1, 16, 3, 1, 16>', 'conv_rows_k<1, 0, 16, 0, true, 3, 1, 4>'), 60, 1, 62, 16, 3, 1, 2, gate=0.3, layout=(1, 1)),
    _c("g.bd.f1", ('conv2d_bf16_k<16, 16, 3, 1, 16>', 'conv_direct_k<16, 0, 8, 8, false>'), 62, 16, 64, 8, 3, 1, 2, co1=8, gate=0.3, drop=(18, 100, 2), layout=(1, 0)),
    _c("g.bd.u1b", ('conv2d_bf16_k<8, 16, 4, 2, 16>', 'conv_direct_k<8, 0, 16, 0, false>'), 64, 8, 34, 16, 4, 2, 3, gate=0.3),
    _c("g.bd.u1a", ('conv2d_bf16_k<16, 32, 3, 1, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 34, 16, 36, 32, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.mid", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 16, false>'), 36, 32, 38, 16, 3, 1, 2, co1=16, gate=0.3, drop=(8, 54, 2), layout=(1, 0)),
    _c("g.bd.u2b", ('conv2d_bf16_k<16, 32, 4, 2, 16>', 'conv_direct_k<16, 0, 32, 0, false>'), 38, 16, 21, 32, 4, 2, 3, gate=0.3),
    _c("g.bd.u2a", ('conv2d_bf16_k<32, 16, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 0, false>'), 21, 32, 23, 16, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.d2b", ('convT2d_bf16_k<16, 16, 12, 2>', 'convT_direct_k<16, 16, 0, 16>'), 23, 16, 48, 16, 4, 2, 0, T=True, gate=0.3, add=(38, 5)),
    _c("g.bd.d2a", ('conv2d_bf16_k<16, 8, 3, 1, 16>', 'conv_direct_k<16, 0, 8, 0, false>'), 48, 16, 50, 8, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("g.bd.d1b", ('convT2d_bf16_k<8, 8, 12, 2>', 'convT_direct_k<8, 8, 0, 8>'), 50, 8, 102, 8, 4, 2, 0, T=True, gate=0.3, add=(64, 20)),
    _c("g.bd.d1a", ('conv2d_bf16_k<8, 8, 3, 1, 16>', 'conv_direct_k<8, 0, 8, 0, true>'), 102, 8, 104, 8, 3, 1, 2, gate=0.3, layout=(1, 1)),
    _c("g.bd.c0", ('conv2d_bf16_k<8, 1, 3, 1, 16>', 'conv_rows_k<8, 0, 1, 0, true, 3, 1, 4>'), 104, 8, 96, 1, 3, 1, -4, layout=(1, 1)),
    _c("d.bd.p2", ('conv_bf16_k<1, 32, 1, 1, 12, true>', None), 20, 1, 20, 32, 1, 1, 0, gate=0.3, layout=(1, None)),
    _c("d.bd.p1", ('conv_bf16_k<32, 32, 1, 1, 12, true>', None), 20, 32, 20, 32, 1, 1, 0, gate=0.09, layout=(1, None)),
    _c("d.bd.d3b", ('convT2d_bf16_k<32, 32, 12, 2>', 'convT_direct_k<32, 32, 0, 8>'), 20, 32, 43, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d3a", ('conv2d_bf16_k<32, 32, 3, 1, 16>', 'conv_direct_k<32, 0, 32, 0, false>'), 43, 32, 45, 32, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("d.bd.d2b", ('convT2d_bf16_k<32, 32, 12, 2>', 'convT_direct_k<32, 32, 0, 8>'), 45, 32, 92, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d2a", ('conv2d_bf16_k<32, 16, 3, 1, 16>', 'conv_direct_k<32, 0, 16, 0, false>'), 92, 32, 94, 16, 3, 1, 2, gate=0.3, layout=(1, 0)),
    _c("d.bd.hack", ('conv2d_bf16_k<16, 1, 3, 1, 16>', 'conv_direct_k<16, 0, 1, 0, true>'), 94, 16, 96, 1, 3, 1, 2, layout=(1, 1)),
]
BWW = [
    _b("g.bww.f2", ('bww2d_bf16_k<1, 16, 3, 1, 8, 8>', 'bww_mfma_k<3, 1>'), 98, 16, 96, 1, 3, 1, 0),
    _b("g.bww.f1", ('bww2d_bf16_k<16, 16, 3, 1, 8, 8>', 'bww_mfma_k<3, 1>'), 100, 8, 98, 16, 3, 1, 0, ci1=8, in1=(126, 14)),
    _b("g.bww.u1b", ('bww2d_bf16_k<8, 16, 4, 2, 8, 8>', 'bww_mfma_k<2, 1>'), 100, 8, 50, 16, 4, 2, 1),
    _b("g.bww.u1a", ('bww2d_bf16_k<32, 16, 3, 1, 8, 8>', 'bww_mfma_k<6, 1>'), 52, 32, 50, 16, 3, 1, 0),
    _b("g.bww.mid", ('bww2d_bf16_k<32, 32, 3, 1, 8, 8>', 'bww_mfma_k<6, 2>'), 54, 16, 52, 32, 3, 1, 0, ci1=16, in1=(60, 3)),
    _b("g.bww.u2b", ('bww2d_bf16_k<16, 32, 4, 2, 8, 8>', 'bww_mfma_k<3, 2>'), 54, 16, 27, 32, 4, 2, 1),
    _b("g.bww.u2a", ('bww2d_bf16_k<16, 32, 3, 1, 8, 8>', 'bww_mfma_k<3, 2>'), 29, 16, 27, 32, 3, 1, 0),
    _b("g.bww.d2b", ('bww2d_bf16_k<16, 16, 4, 2, 8, 8>', 'bww_mfma_k<3, 1>'), 60, 16, 29, 16, 4, 2, 0),
    _b("g.bww.d2a", ('bww2d_bf16_k<8, 16, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 62, 8, 60, 16, 3, 1, 0),
    _b("g.bww.d1b", ('bww2d_bf16_k<8, 8, 4, 2, 8, 8>', 'bww_mfma_k<2, 1>'), 126, 8, 62, 8, 4, 2, 0),
    _b("g.bww.d1a", ('bww2d_bf16_k<8, 8, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 128, 8, 126, 8, 3, 1, 0),
    _b("g.bww.c0", ('bww2d_bf16_k<1, 8, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 132, 1, 128, 8, 3, 1, 0),
    _b("g.bww.f2", ('bww2d_bf16_k<1, 16, 3, 1, 8, 8>', 'bww_mfma_k<3, 1>'), 62, 16, 60, 1, 3, 1, 0),
    _b("g.bww.f1", ('bww2d_bf16_k<16, 16, 3, 1, 8, 8>', 'bww_mfma_k<3, 1>'), 64, 8, 62, 16, 3, 1, 0, ci1=8, in1=(102, 20)),
    _b("g.bww.u1b", ('bww2d_bf16_k<8, 16, 4, 2, 8, 8>', 'bww_mfma_k<2, 1>'), 64, 8, 34, 16, 4, 2, 3),
    _b("g.bww.u1a", ('bww2d_bf16_k<32, 16, 3, 1, 8, 8>', 'bww_mfma_k<6, 1>'), 36, 32, 34, 16, 3, 1, 0),
    _b("g.bww.mid", ('bww2d_bf16_k<32, 32, 3, 1, 8, 8>', 'bww_mfma_k<6, 2>'), 38, 16, 36, 32, 3, 1, 0, ci1=16, in1=(48, 5)),
    _b("g.bww.u2b", ('bww2d_bf16_k<16, 32, 4, 2, 8, 8>', 'bww_mfma_k<3, 2>'), 38, 16, 21, 32, 4, 2, 3),
    _b("g.bww.u2a", ('bww2d_bf16_k<16, 32, 3, 1, 8, 8>', 'bww_mfma_k<3, 2>'), 23, 16, 21, 32, 3, 1, 0),
    _b("g.bww.d2b", ('bww2d_bf16_k<16, 16, 4, 2, 8, 8>', 'bww_mfma_k<3, 1>'), 48, 16, 23, 16, 4, 2, 0),
    _b("g.bww.d2a", ('bww2d_bf16_k<8, 16, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 50, 8, 48, 16, 3, 1, 0),
    _b("g.bww.d1b", ('bww2d_bf16_k<8, 8, 4, 2, 8, 8>', 'bww_mfma_k<2, 1>'), 102, 8, 50, 8, 4, 2, 0),
    _b("g.bww.d1a", ('bww2d_bf16_k<8, 8, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 104, 8, 102, 8, 3, 1, 0),
    _b("g.bww.c0", ('bww2d_bf16_k<1, 8, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 96, 1, 104, 8, 3, 1, 6),
    _b("d.bww.p2", ('bww_bf16_k<1, 32, 1, 1, 12, 4, 1>', None), 20, 32, 20, 1, 1, 1, 0),
    _b("d.bww.p1", ('bww_bf16_k<32, 32, 1, 1, 12, 4, 2>', None), 20, 32, 20, 32, 1, 1, 0),
    _b("d.bww.d3b", ('bww2d_bf16_k<32, 32, 4, 2, 8, 8>', 'bww_mfma_k<6, 2>'), 43, 32, 20, 32, 4, 2, 0),
    _b("d.bww.d3a", ('bww2d_bf16_k<32, 32, 3, 1, 8, 8>', 'bww_mfma_k<6, 2>'), 45, 32, 43, 32, 3, 1, 0),
    _b("d.bww.d2b", ('bww2d_bf16_k<32, 32, 4, 2, 8, 8>', 'bww_mfma_k<6, 2>'), 92, 32, 45, 32, 4, 2, 0),
    _b("d.bww.d2a", ('bww2d_bf16_k<16, 32, 3, 1, 8, 8>', 'bww_mfma_k<3, 2>'), 94, 16, 92, 32, 3, 1, 0),
    _b("d.bww.hack", ('bww2d_bf16_k<1, 16, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 96, 1, 94, 16, 3, 1, 0, in0=(132, 18)),
    _b("d.bww.hack", ('bww2d_bf16_k<1, 16, 3, 1, 8, 8>', 'bww_mfma_k<2, 1>'), 96, 1, 94, 16, 3, 1, 0),
]

CONV_BF16, CONV_FP32 = F.select(CONV, 0), F.select(CONV, 1)
BWW_BF16, BWW_FP32 = F.select(BWW, 0), F.select(BWW, 1)


def _ids(rows):
    return [f"{i}-{r['name']}" for i, r in enumerate(rows)]


@pytest.mark.parametrize("case", CONV_BF16, ids=_ids(CONV_BF16))
def test_convolution2d_bf16_notebook_shapes(H, T, oracle_lib, case):
    F.check_conv(H, T, oracle_lib, case, N, IS3D, True, seed=case["n"] + case["co0"])


@pytest.mark.parametrize("case", BWW_BF16, ids=_ids(BWW_BF16))
def test_kernel_gradient2d_bf16_notebook_shapes(H, T, case):
    F.check_bww(H, T, case, N, IS3D, True, seed=case["n"] + case["co"])


@pytest.mark.parametrize("case", CONV_FP32, ids=_ids(CONV_FP32))
def test_convolution2d_fp32_notebook_shapes(H, T, oracle_lib, case):
    F.check_conv(H, T, oracle_lib, case, N, IS3D, False, seed=case["n"] + case["co0"])


@pytest.mark.parametrize("case", BWW_FP32, ids=_ids(BWW_FP32))
def test_kernel_gradient2d_fp32_notebook_shapes(H, T, case):
    F.check_bww(H, T, case, N, IS3D, False, seed=case["n"] + case["co"])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_tables_cover_the_step(H, tmp_path, precision):
    """Every conv / convT / bww launch of the compiled 132^2 batch-64 step has a table case with the same launch key
    (fullsize_cases.launch_key), and every table case is a launch of the step."""
    from transfer_em_amd.cgan import EM2EM
    bf16 = precision == "bf16"
    conv, bww = (CONV_BF16, BWW_BF16) if bf16 else (CONV_FP32, BWW_FP32)
    model = EM2EM(132, "cover", is3d=False, checkpoint_root=str(tmp_path), precision=precision)
    x = torch.randn(N, 1, 132, 132, 1)
    model.train_step(x, x.flip(2))
    keys = {F.launch_key(F.build_conv(H, c, N, IS3D, bf16)[0]) for c in conv}
    keys |= {F.launch_key(F.build_bww(H, c, N, IS3D, bf16)[0]) for c in bww}
    assert len(keys) == len(conv) + len(bww), "two table cases describe the same launch"
    F.assert_tables_cover(model._compiled(N), keys)
