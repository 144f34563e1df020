"""The bf16 train step's own kernel variants at the step's own shapes (BASELINE configs[4]: 3-D 132^3, batch 1, bf16 mixed
precision) against the CPU oracle, one launch at a time: the bf16 twin of test_gpu_fullsize_oracle.py.

CONV and BWW list every convolution, transposed-convolution and kernel-gradient launch of
EM2EM(132, precision="bf16")'s compiled step once (fullsize_cases._c / _b: channel split, extents, k / s / p, the skip
crops behind an input, the cone path's shifted windows and Dropout frames, LeakyReLU, gate, skip-gradient add, keep-mask
mode, split outputs, bias).  Each case checks the kernel symbol and compares the launch with oracle/torch_ops.py (float64)
on the bf16-rounded operands; outputs start NaN-filled, so a voxel the kernel leaves out fails the comparison.
test_tables_cover_the_step holds the tables to the step: a launch the step gains, loses or changes fails it.

Bars (fullsize_cases.py): 6e-3 of the output's largest value for bf16 outputs (test_gpu_bf16.TOL: one bf16 ulp at the top
of the range, independent of the tensor's size), 2e-5 for the fp32 kernel-gradient slabs (exact products of bf16 values;
the error is the fp32 summation order, which grows like the entries themselves).  Rows of at most 2^22 output elements
also hold every stored bf16 element to the rounded float64 reference (fullsize_cases.exact_checked, bf16_exact.py); the
larger ones keep the max-norm bar only, and test_bf16_exact.py checks that each of their kernels runs in a case that
gets the element-by-element check.  Parity unpinned (oracle/README.md)."""
import pytest
import torch

import fullsize_cases as F
from fullsize_cases import _b, _c

pytestmark = pytest.mark.gpu
N, IS3D = 1, True


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
    _c("g.c0", 'c1_mfma_h_k<8, false, 0>', 132, 1, 128, 8, 3, 1, 0, slope=0.3),
    _c("g.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 8>', 128, 8, 126, 8, 3, 1, 0, slope=0.3),
    _c("g.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 126, 8, 62, 8, 4, 2, 0, slope=0.3),
    _c("g.d2a", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 62, 8, 60, 16, 3, 1, 0, slope=0.3),
    _c("g.d2b", 'conv3_bf16_k<16, 16, 4, 2, 4, false, 8>', 60, 16, 29, 16, 4, 2, 0, slope=0.3),
    _c("g.u2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 29, 16, 27, 32, 3, 1, 0, slope=0.3),
    _c("g.u2b", 'convT_bf16_k<32, 16, 12, 1, 1>', 27, 32, 54, 16, 4, 2, 1, T=True, slope=0.3, drop=(0, 54, 2)),
    _c("g.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 54, 16, 52, 32, 3, 1, 0, ci1=16, in1=(60, 3), slope=0.3),
    _c("g.u1a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 8>', 52, 32, 50, 16, 3, 1, 0, slope=0.3),
    _c("g.u1b", 'convT_bf16_k<16, 8, 12, 1, 1>', 50, 16, 100, 8, 4, 2, 1, T=True, slope=0.3, drop=(0, 100, 2)),
    _c("g.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 8>', 100, 8, 98, 16, 3, 1, 0, ci1=8, in1=(126, 14), slope=0.3),
    _c("g.f2", 'c1out_h_k<16, false, false>', 98, 16, 96, 1, 3, 1, 0),
    _c("g.c0", 'c1_mfma_h_k<8, false, 0>', 96, 1, 104, 8, 3, 1, 6, slope=0.3),
    _c("g.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 8>', 104, 8, 102, 8, 3, 1, 0, slope=0.3),
    _c("g.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 102, 8, 50, 8, 4, 2, 0, slope=0.3),
    _c("g.d2a", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 50, 8, 48, 16, 3, 1, 0, slope=0.3),
    _c("g.d2b", 'conv3_bf16_k<16, 16, 4, 2, 4, false, 8>', 48, 16, 23, 16, 4, 2, 0, slope=0.3),
    _c("g.u2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 23, 16, 21, 32, 3, 1, 0, slope=0.3),
    _c("g.u2b", 'convT_bf16_k<32, 16, 12, 1, 1>', 21, 32, 38, 16, 4, 2, 3, T=True, slope=0.3, drop=(8, 54, 2)),
    _c("g.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 38, 16, 36, 32, 3, 1, 0, ci1=16, in1=(48, 5), slope=0.3),
    _c("g.u1a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 8>', 36, 32, 34, 16, 3, 1, 0, slope=0.3),
    _c("g.u1b", 'convT_bf16_k<16, 8, 12, 1, 1>', 34, 16, 64, 8, 4, 2, 3, T=True, slope=0.3, drop=(18, 100, 2)),
    _c("g.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 8>', 64, 8, 62, 16, 3, 1, 0, ci1=8, in1=(102, 20), slope=0.3),
    _c("g.f2", 'c1out_h_k<16, false, false>', 62, 16, 60, 1, 3, 1, 0),
    _c("d.d1a", 'c1_mfma_h_k<8, false, 0>', 96, 1, 94, 8, 3, 1, 0, in0=(132, 18), slope=0.3),
    _c("d.d1b", 'conv3_bf16_k<8, 8, 4, 2, 8, false, 8>', 94, 8, 46, 8, 4, 2, 0, slope=0.3),
    _c("d.hack", 'conv3_bf16_k<8, 16, 3, 1, 8, false, 8>', 46, 8, 44, 16, 3, 1, 0, slope=0.3),
    _c("d.d2a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 8>', 44, 16, 42, 32, 3, 1, 0, slope=0.3),
    _c("d.d2b", 'conv_bf16_k<32, 32, 4, 2, 12, false>', 42, 32, 20, 32, 4, 2, 0, slope=0.3),
    _c("d.d3a", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 8>', 20, 32, 18, 32, 3, 1, 0, slope=0.3),
    _c("d.d3b", 'conv_bf16_k<32, 32, 4, 2, 12, false>', 18, 32, 8, 32, 4, 2, 0, slope=0.09),
    _c("d.p1", 'conv_bf16_k<32, 32, 1, 1, 12, true>', 8, 32, 8, 32, 1, 1, 0, slope=0.3),
    _c("d.p2", 'conv_bf16_k<32, 1, 1, 1, 12, true>', 8, 32, 8, 1, 1, 1, 0, bias=True),
    _c("d.d1a", 'c1_mfma_h_k<8, false, 0>', 96, 1, 94, 8, 3, 1, 0, slope=0.3),
    _c("g.bd.f2", 'c1_mfma_h_k<16, true, 1>', 96, 1, 98, 16, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 5>', 98, 16, 100, 8, 3, 1, 2, co1=8, gate=0.3, drop=(0, 100, 2), layout=1),
    _c("g.bd.u1b", 'conv3_bf16_k<8, 16, 4, 2, 8, false, 1>', 100, 8, 50, 16, 4, 2, 1, gate=0.3),
    _c("g.bd.u1a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 1>', 50, 16, 52, 32, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 5>', 52, 32, 54, 16, 3, 1, 2, co1=16, gate=0.3, drop=(0, 54, 2), layout=1),
    _c("g.bd.u2b", 'conv3_bf16_k<16, 32, 4, 2, 4, true, 1>', 54, 16, 27, 32, 4, 2, 1, gate=0.3),
    _c("g.bd.u2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 27, 32, 29, 16, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.d2b", 'convT_bf16_k<16, 16, 12, 1, 2>', 29, 16, 60, 16, 4, 2, 0, T=True, gate=0.3, add=(54, 3)),
    _c("g.bd.d2a", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 60, 16, 62, 8, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 62, 8, 126, 8, 4, 2, 0, T=True, gate=0.3, add=(100, 14)),
    _c("g.bd.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 1>', 126, 8, 128, 8, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.f2", 'c1_mfma_h_k<16, true, 1>', 60, 1, 62, 16, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.f1", 'conv3_bf16_k<16, 16, 3, 1, 8, false, 5>', 62, 16, 64, 8, 3, 1, 2, co1=8, gate=0.3, drop=(18, 100, 2), layout=1),
    _c("g.bd.u1b", 'conv3_bf16_k<8, 16, 4, 2, 8, false, 1>', 64, 8, 34, 16, 4, 2, 3, gate=0.3),
    _c("g.bd.u1a", 'conv3_bf16_k<16, 32, 3, 1, 4, false, 1>', 34, 16, 36, 32, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.mid", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 5>', 36, 32, 38, 16, 3, 1, 2, co1=16, gate=0.3, drop=(8, 54, 2), layout=1),
    _c("g.bd.u2b", 'conv3_bf16_k<16, 32, 4, 2, 4, true, 1>', 38, 16, 21, 32, 4, 2, 3, gate=0.3),
    _c("g.bd.u2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 21, 32, 23, 16, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.d2b", 'convT_bf16_k<16, 16, 12, 1, 2>', 23, 16, 48, 16, 4, 2, 0, T=True, gate=0.3, add=(38, 5)),
    _c("g.bd.d2a", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 48, 16, 50, 8, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 50, 8, 102, 8, 4, 2, 0, T=True, gate=0.3, add=(64, 20)),
    _c("g.bd.d1a", 'conv3_bf16_k<8, 8, 3, 1, 8, false, 1>', 102, 8, 104, 8, 3, 1, 2, gate=0.3, layout=1),
    _c("g.bd.c0", 'c1out_h_k<8, true, false>', 104, 8, 96, 1, 3, 1, -4, layout=1),
    _c("d.bd.p2", 'conv_bf16_k<1, 32, 1, 1, 12, true>', 8, 1, 8, 32, 1, 1, 0, gate=0.3, layout=1),
    _c("d.bd.p1", 'conv_bf16_k<32, 32, 1, 1, 12, true>', 8, 32, 8, 32, 1, 1, 0, gate=0.09, layout=1),
    _c("d.bd.d3b", 'convT_bf16_k<32, 32, 12, 1, 2>', 8, 32, 18, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d3a", 'conv3_bf16_k<32, 32, 3, 1, 4, true, 1>', 18, 32, 20, 32, 3, 1, 2, gate=0.3, layout=1),
    _c("d.bd.d2b", 'convT_bf16_k<32, 32, 12, 1, 2>', 20, 32, 42, 32, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d2a", 'conv3_bf16_k<32, 16, 3, 1, 4, false, 1>', 42, 32, 44, 16, 3, 1, 2, gate=0.3, layout=1),
    _c("d.bd.hack", 'conv3_bf16_k<16, 8, 3, 1, 8, false, 1>', 44, 16, 46, 8, 3, 1, 2, gate=0.3, layout=1),
    _c("d.bd.d1b", 'convT_bf16_k<8, 8, 12, 1, 2>', 46, 8, 94, 8, 4, 2, 0, T=True, gate=0.3),
    _c("d.bd.d1a", 'c1out_h_k<8, true, false>', 94, 8, 96, 1, 3, 1, 2, layout=1),
]
BWW = [
    _b("g.bww.f2", 'bww_c1m_h_k<16>', 98, 16, 96, 1, 3, 1, 0),
    _b("g.bww.f1", 'bww_bf16_k<16, 16, 3, 1, 12, 4, 27>', 100, 8, 98, 16, 3, 1, 0, ci1=8, in1=(126, 14)),
    _b("g.bww.u1b", 'bww_bf16_k<8, 16, 4, 2, 12, 4, 32>', 100, 8, 50, 16, 4, 2, 1),
    _b("g.bww.u1a", 'bww_bf16_k<32, 16, 3, 1, 12, 4, 54>', 52, 32, 50, 16, 3, 1, 0),
    _b("g.bww.mid", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 54, 16, 52, 32, 3, 1, 0, ci1=16, in1=(60, 3)),
    _b("g.bww.u2b", 'bww_bf16_k<16, 32, 4, 2, 12, 4, 32>', 54, 16, 27, 32, 4, 2, 1),
    _b("g.bww.u2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 29, 16, 27, 32, 3, 1, 0),
    _b("g.bww.d2b", 'bww_bf16_k<16, 16, 4, 2, 12, 4, 64>', 60, 16, 29, 16, 4, 2, 0),
    _b("g.bww.d2a", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 62, 8, 60, 16, 3, 1, 0),
    _b("g.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 126, 8, 62, 8, 4, 2, 0),
    _b("g.bww.d1a", 'bww_bf16_k<8, 8, 3, 1, 12, 4, 14>', 128, 8, 126, 8, 3, 1, 0),
    _b("g.bww.c0", 'bww_c1m_h_k<8>', 132, 1, 128, 8, 3, 1, 0),
    _b("g.bww.f2", 'bww_c1m_h_k<16>', 62, 16, 60, 1, 3, 1, 0),
    _b("g.bww.f1", 'bww_bf16_k<16, 16, 3, 1, 12, 4, 27>', 64, 8, 62, 16, 3, 1, 0, ci1=8, in1=(102, 20)),
    _b("g.bww.u1b", 'bww_bf16_k<8, 16, 4, 2, 12, 4, 32>', 64, 8, 34, 16, 4, 2, 3),
    _b("g.bww.u1a", 'bww_bf16_k<32, 16, 3, 1, 12, 4, 54>', 36, 32, 34, 16, 3, 1, 0),
    _b("g.bww.mid", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 38, 16, 36, 32, 3, 1, 0, ci1=16, in1=(48, 5)),
    _b("g.bww.u2b", 'bww_bf16_k<16, 32, 4, 2, 12, 4, 32>', 38, 16, 21, 32, 4, 2, 3),
    _b("g.bww.u2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 23, 16, 21, 32, 3, 1, 0),
    _b("g.bww.d2b", 'bww_bf16_k<16, 16, 4, 2, 12, 4, 64>', 48, 16, 23, 16, 4, 2, 0),
    _b("g.bww.d2a", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 50, 8, 48, 16, 3, 1, 0),
    _b("g.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 102, 8, 50, 8, 4, 2, 0),
    _b("g.bww.d1a", 'bww_bf16_k<8, 8, 3, 1, 12, 4, 14>', 104, 8, 102, 8, 3, 1, 0),
    _b("g.bww.c0", 'bww_c1m_h_k<8>', 96, 1, 104, 8, 3, 1, 6),
    _b("d.bww.p2", 'bww_bf16_k<1, 32, 1, 1, 12, 4, 1>', 8, 32, 8, 1, 1, 1, 0),
    _b("d.bww.p1", 'bww_bf16_k<32, 32, 1, 1, 12, 4, 2>', 8, 32, 8, 32, 1, 1, 0),
    _b("d.bww.d3b", 'bww_bf16_k<32, 32, 4, 2, 12, 4, 32>', 18, 32, 8, 32, 4, 2, 0),
    _b("d.bww.d3a", 'bww_bf16_k<32, 32, 3, 1, 12, 4, 27>', 20, 32, 18, 32, 3, 1, 0),
    _b("d.bww.d2b", 'bww_bf16_k<32, 32, 4, 2, 12, 4, 32>', 42, 32, 20, 32, 4, 2, 0),
    _b("d.bww.d2a", 'bww_bf16_k<16, 32, 3, 1, 12, 4, 27>', 44, 16, 42, 32, 3, 1, 0),
    _b("d.bww.hack", 'bww_bf16_k<8, 16, 3, 1, 12, 4, 14>', 46, 8, 44, 16, 3, 1, 0),
    _b("d.bww.d1b", 'bww_bf16_k<8, 8, 4, 2, 12, 4, 32>', 94, 8, 46, 8, 4, 2, 0),
    _b("d.bww.d1a", 'bww_c1m_h_k<8>', 96, 1, 94, 8, 3, 1, 0, in0=(132, 18)),
    _b("d.bww.d1a", 'bww_c1m_h_k<8>', 96, 1, 94, 8, 3, 1, 0),
]


def _ids(rows):
    return [f"{i}-{r['name']}" for i, r in enumerate(rows)]


@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_convolution_bf16_step_shapes(H, T, oracle_lib, case):
    F.check_conv(H, T, oracle_lib, case, N, IS3D, True, seed=case["n"] + case["co0"])


@pytest.mark.parametrize("case", BWW, ids=_ids(BWW))
def test_kernel_gradient_bf16_step_shapes(H, T, case):
    F.check_bww(H, T, case, N, IS3D, True, seed=case["n"] + case["co"])


def test_tables_cover_the_step(H, tmp_path):
    """Every conv / convT / bww launch of the compiled 132^3 bf16 step has a table case with the same launch key
    (fullsize_cases.launch_key), and every table case is a launch of the step."""
    from transfer_em_amd.cgan import EM2EM
    model = EM2EM(132, "cover", checkpoint_root=str(tmp_path), precision="bf16")
    x = torch.randn(N, 132, 132, 132, 1)
    model.train_step(x, x.flip(1))
    keys = {F.launch_key(F.build_conv(H, c, N, IS3D, True)[0]) for c in CONV}
    keys |= {F.launch_key(F.build_bww(H, c, N, IS3D, True)[0]) for c in BWW}
    assert len(keys) == len(CONV) + len(BWW), "two table cases describe the same launch"
    F.assert_tables_cover(model._compiled(N), keys)
