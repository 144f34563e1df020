"""The span limits of the convolution kernels as a table, and the argument structs that sit on either side of each.

One `Row` per (kernel, operand, limited quantity, placement).  The limits were read off the dispatch functions and the
kernels' address arithmetic ("Span limits of the convolution kernels"), not probed from the library; `why`
says in one line what in the kernel needs the limit.  tests/test_span_routing.py asks the library's dry queries about
both sides of every row, tests/test_gpu_span_limits.py runs them.

Quantities (elements of the operand's type):
  view   elements from the first of the view to one past its last (tem_common.h: view_span)
  image  the same over one image: (D-1) sD + (H-1) sH + (W-1) sW + C
  row    the same over one z-plane: (H-1) sH + (W-1) sW + C
  sN     the image stride by itself (a kernel may hold it as an int even where N == 1)
  keep   elements of the dropout frame, N dD dH dW C: one keep bit each
Placements: how the quantity gets there with small extents -- exactly one operand is stretched, the others stay dense.
  image  N = 3, sN stretched: the way a large tile batch reaches a limit; the last image carries the large offsets
  plane  N = 1, sD stretched (sH for a 2-D operand): the large offsets lie inside one image
  row    N = 1, sH stretched with the planes interleaved (sD = one row): the large offsets lie inside one plane
  sN     N = 1 with a huge sN that no address uses
  frame  a dropout frame (drop_dims) larger than the output, whose window (drop_org) is the frame's far corner; no
         operand is stretched
"""
import ctypes as C
from collections import namedtuple

Row = namedtuple("Row", "family kernel geom operand quantity limit place fallback why")
Row.id = property(lambda r: f"{r.kernel}-{r.geom}-{r.operand}-{r.quantity}-{r.place}")
View = namedtuple("View", "N D H W C sN sD sH sW")
MAX_SLABS = 8192

# ------------------------------------------------------------------------------------------------ geometries
# entry: conv | convT | bww | bww_wino (fp32), conv_h | convT_h | bww_h (bf16).  dims = (D, H, W) of in0: the smallest
# ragged shapes of the same family's cases in test_gpu_ops / test_gpu_wino / test_gpu_bf16 / test_gpu_bf16_2d.
def _g(entry, ci, co, k, s, p, dims, ci1=0, co1=0, flip=False, wino=False, slope=0.3, gate=False, add=False, keep=0):
    return dict(entry=entry, ci=ci, ci1=ci1, co=co, co1=co1, k=k, s=s, p=p, dims=dims, flip=flip, wino=wino, slope=slope,
                gate=gate, add=add, keep=keep, is3d=dims[0] > 1, esz=2 if entry.endswith("_h") else 4)


GEOM = {
    # ---- fp32
    "s2": _g("conv", 8, 16, 4, 2, 1, (12, 14, 16), slope=1.0, gate=True, add=True),     # input-gradient of g.u1b's kind
    "c1out": _g("conv", 16, 1, 3, 1, 0, (10, 12, 14), slope=1.0),                      # g.f2
    "c1out_bd": _g("conv", 8, 1, 3, 1, 2, (10, 12, 14), flip=True, slope=1.0, gate=True),   # input-gradient of g.c0: padded
    "wino": _g("conv", 8, 16, 3, 1, 0, (10, 12, 14), ci1=8, wino=True),                 # g.f1: concat 8 + 8
    "wino_bd": _g("conv", 16, 16, 3, 1, 2, (10, 12, 14), flip=True, wino=True, slope=1.0, gate=True),
    "wino_keep": _g("conv", 16, 8, 3, 1, 2, (10, 12, 14), co1=8, flip=True, wino=True, slope=1.0, gate=True, keep=2),
    "c1m": _g("conv", 1, 8, 3, 1, 0, (10, 12, 16)),                                    # g.c0
    "c1m_bd": _g("conv", 1, 16, 3, 1, 2, (10, 12, 16), flip=True, slope=1.0, gate=True),    # input-gradient of g.f2
    "c1s": _g("conv", 1, 8, 3, 1, 0, (10, 12, 15)),                                    # W % 4 != 0: the VALU stencil
    "c1s_g": _g("conv", 1, 8, 3, 1, 0, (10, 12, 15), slope=1.0, gate=True),
    "convT": _g("convT", 16, 8, 4, 2, 1, (5, 6, 7)),                                   # g.u1b
    "convT_bd": _g("convT", 8, 8, 4, 2, 0, (5, 6, 7), slope=1.0, gate=True, add=True),     # input-gradient of g.d1b
    "convT_keep": _g("convT", 16, 8, 4, 2, 1, (5, 6, 7), keep=2),
    "lds": _g("conv", 16, 32, 3, 1, 0, (9, 10, 11)),                                   # g.u2a below the Winograd threshold
    "lds_cat": _g("conv", 16, 32, 3, 1, 0, (9, 10, 11), ci1=16),                        # g.mid: concat 16 + 16
    "lds_bd": _g("conv", 32, 16, 3, 1, 2, (7, 8, 9), co1=16, flip=True, slope=1.0, gate=True),   # its input-gradient: split
    "lds_add": _g("conv", 16, 16, 3, 1, 0, (9, 10, 11), slope=1.0, add=True),
    "wbww": _g("bww_wino", 16, 16, 3, 1, 0, (10, 12, 14)),
    "wbww_cat": _g("bww_wino", 8, 16, 3, 1, 0, (10, 12, 14), ci1=8),
    "bc1": _g("bww", 1, 8, 3, 1, 0, (10, 12, 16)),
    "bs2": _g("bww", 16, 16, 4, 2, 0, (12, 13, 14)),
    # ---- bf16
    "h3": _g("conv_h", 8, 8, 3, 1, 0, (10, 12, 14)),
    "h3_bd": _g("conv_h", 16, 16, 3, 1, 2, (8, 9, 10), slope=1.0, gate=True),
    "h1": _g("conv_h", 32, 32, 1, 1, 0, (5, 6, 7), slope=1.0, gate=True, add=True),      # 1x1x1: the generic bf16 kernel
    "h1_keep": _g("conv_h", 32, 32, 1, 1, 0, (5, 6, 7), keep=2),
    "h3_cat": _g("conv_h", 8, 16, 3, 1, 0, (10, 12, 14), ci1=8),                        # concat 8 + 8
    "h3_split": _g("conv_h", 16, 8, 3, 1, 0, (10, 12, 14), co1=8, slope=1.0),           # split 8 + 8
    "h3_add": _g("conv_h", 16, 16, 3, 1, 2, (8, 9, 10), slope=1.0, gate=True, add=True),
    "h2d": _g("conv_h", 8, 8, 3, 1, 0, (1, 12, 14)),
    "h2d_cat": _g("conv_h", 8, 16, 3, 1, 0, (1, 12, 14), ci1=8),
    "h2d_split": _g("conv_h", 16, 8, 3, 1, 0, (1, 12, 14), co1=8, slope=1.0),
    "h2d_ep": _g("conv_h", 16, 16, 3, 1, 0, (1, 12, 14), slope=1.0, gate=True, add=True),
    "hT_ep": _g("convT_h", 16, 8, 4, 2, 1, (5, 6, 7), slope=1.0, gate=True, add=True),
    "hT2d_ep": _g("convT_h", 16, 8, 4, 2, 1, (1, 6, 7), slope=1.0, gate=True, add=True),
    "hc1m_g": _g("conv_h", 1, 8, 3, 1, 0, (10, 12, 16), slope=1.0, gate=True),
    "hc1out_g": _g("conv_h", 16, 1, 3, 1, 0, (10, 12, 14), slope=1.0, gate=True),
    "hbww_cat": _g("bww_h", 8, 8, 3, 1, 0, (10, 12, 14), ci1=8),
    "hbww2d_cat": _g("bww_h", 8, 8, 3, 1, 0, (1, 12, 14), ci1=8),
    "hT": _g("convT_h", 16, 8, 4, 2, 1, (5, 6, 7)),
    "hT2d": _g("convT_h", 16, 8, 4, 2, 1, (1, 6, 7)),
    "hc1m": _g("conv_h", 1, 8, 3, 1, 0, (10, 12, 16)),
    "hc1out": _g("conv_h", 16, 1, 3, 1, 0, (10, 12, 14), slope=1.0),
    "hbww": _g("bww_h", 8, 8, 3, 1, 0, (10, 12, 14)),
    "hbww2d": _g("bww_h", 8, 8, 3, 1, 0, (1, 12, 14)),
    "hbc1": _g("bww_h", 1, 8, 3, 1, 0, (10, 12, 16)),
}

B28, B29, B30, B31, B32, B33 = (1 << n for n in (28, 29, 30, 31, 32, 33))
BYTES = "byte offset of a buffer load / store: a signed 32-bit VGPR (elements x 4 < 2^31)"
ELEMS = "element offset n sN + z sD + y sH + x sW + c is a 32-bit int"
SN = "the kernel's argument struct holds sN as an int32"

LIMITS = []


def _rows(family, kernel, geom, rows):
    for operand, quantity, limit, places, fallback, why in rows:
        for place in places:
            LIMITS.append(Row(family, kernel, geom, operand, quantity, limit, place, fallback, why))


# conv_s2.hip: every global read goes through a buffer descriptor over the whole view
_rows("conv_s2.hip", "conv_s2_k", "s2", [
    ("in0", "view", B29, ("image", "plane"), "conv_direct_k", BYTES + "; descriptor range in_bytes is an int"),
    ("gate", "view", B29, ("image",), "conv_direct_k", BYTES),
    ("add", "view", B29, ("image",), "conv_direct_k", BYTES),
    ("out0", "view", B31, ("image",), "conv_direct_k", ELEMS + " added to the 64-bit base (stricter in0 limit aside)"),
])
# c1out_mfma.hip
_rows("c1out_mfma.hip", "c1out_mfma_k", "c1out", [
    ("in0", "view", B29, ("image", "plane"), "c1_stencil_k", BYTES),
    ("out0", "view", B29, ("image", "plane"), "c1_stencil_k", BYTES),
])
_rows("c1out_mfma.hip", "c1out_mfma_k", "c1out_bd", [
    ("in0", "view", B28, ("image", "plane"), "c1_stencil_k",
     "a plane of the zero padding adds 2^30 bytes to a valid offset; the sum must lie past the descriptor's range "
     "(TIGHTENED here: was 2^29)"),
    ("gate", "view", B29, ("image",), "c1_stencil_k", BYTES),
])
# wino.hip: images are rebased in 64 bits ((size_t) n sN), planes by an int (z sD), offsets inside a plane are bytes
_rows("wino.hip", "wino_conv_k", "wino", [
    ("in0", "view", B31, ("image",), "conv_direct_k", "plane base z sD is a 32-bit int added to the image's pointer"),
    ("in0", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("in0", "row", B29, ("row",), "conv_lds_k", "LDS-DMA offset inside a plane is a byte offset in a signed 32-bit VGPR (NEW here)"),
    ("in1", "view", B31, ("image",), "conv_direct_k", "plane base z sD is a 32-bit int added to the image's pointer"),
    ("in1", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("in1", "row", B29, ("row",), "conv_lds_k", "LDS-DMA offset inside a plane is a byte offset in a signed 32-bit VGPR (NEW here)"),
    ("out0", "view", B31, ("image",), "conv_direct_k", "stricter than needed: only sN and the image span are used"),
    ("out0", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("out0", "image", B29, ("plane",), "conv_lds_k", BYTES + " inside the image's descriptor"),
])
_rows("wino.hip", "wino_conv_k", "wino_bd", [
    ("gate", "view", B31, ("image",), "conv_direct_k", "stricter than needed: only sN and the image span are used"),
    ("gate", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("gate", "image", B29, ("plane",), "conv_lds_k", BYTES + " inside the image's descriptor"),
])
_rows("wino.hip", "wino_conv_k", "wino_keep", [
    ("out1", "view", B31, ("image",), "conv_direct_k", ELEMS + " inside the image"),
    ("out1", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("keep", "keep", B32, ("frame",), "conv_lds_k", "the keep byte's voxel index is 32-bit unsigned arithmetic"),
])
# stencil_c1.hip
_rows("stencil_c1.hip", "c1_mfma_k", "c1m", [
    ("in0", "view", B29, ("image", "plane"), "c1_stencil_k", BYTES + " over the whole view"),
    ("out0", "image", B29, ("plane",), "c1_stencil_k", BYTES + " inside the image's descriptor"),
    ("out0", "view", B31, ("image",), "conv_direct_k", "stricter than needed: images are rebased in 64 bits"),
])
_rows("stencil_c1.hip", "c1_mfma_k", "c1m_bd", [
    ("gate", "image", B29, ("plane",), "c1_stencil_k", BYTES + " inside the image's descriptor"),
    ("gate", "view", B31, ("image",), "conv_direct_k", "stricter than needed: images are rebased in 64 bits"),
])
_rows("stencil_c1.hip", "c1_stencil_k", "c1s", [
    ("in0", "view", B31, ("image", "plane"), "conv_direct_k", ELEMS),
    ("out0", "view", B31, ("image",), "conv_direct_k", ELEMS),
])
_rows("stencil_c1.hip", "c1_stencil_k", "c1s_g", [("gate", "view", B31, ("image",), "conv_direct_k", ELEMS)])
# convT_mfma.hip
_rows("convT_mfma.hip", "convT_mfma_k", "convT", [
    ("in0", "view", B31, ("image", "plane"), "convT_direct_k", ELEMS),
    ("out0", "view", B31, ("image",), "convT_direct_k", ELEMS),
])
_rows("convT_mfma.hip", "convT_mfma_k", "convT_bd", [
    ("gate", "view", B29, ("image",), "convT_direct_k", BYTES),
    ("add", "view", B29, ("image",), "convT_direct_k", BYTES),
])
_rows("convT_mfma.hip", "convT_mfma_k", "convT_keep", [
    ("keep", "keep", B32, ("frame",), "convT_direct_k", "the keep byte's voxel index is 32-bit unsigned arithmetic"),
])
# conv_lds.hip
_rows("conv_lds.hip", "conv_lds_k", "lds", [
    ("in0", "view", B31, ("image", "plane"), "conv_direct_k", ELEMS),
    ("in0", "sN", B31, ("sN",), "conv_direct_k", SN),
    ("out0", "view", B31, ("image",), "conv_direct_k", ELEMS),
    ("out0", "sN", B31, ("sN",), "conv_direct_k", SN),
])
_rows("conv_lds.hip", "conv_lds_k", "lds_cat", [("in1", "view", B31, ("image",), "conv_direct_k", ELEMS),
                                                 ("in1", "sN", B31, ("sN",), "conv_direct_k", SN)])
_rows("conv_lds.hip", "conv_lds_k", "lds_bd", [("out1", "view", B31, ("image",), "conv_direct_k", ELEMS),
                                                ("out1", "sN", B31, ("sN",), "conv_direct_k", SN),
                                                ("gate", "view", B31, ("image",), "conv_direct_k", ELEMS),
                                                ("gate", "sN", B31, ("sN",), "conv_direct_k", SN)])
_rows("conv_lds.hip", "conv_lds_k", "lds_add", [("add", "view", B31, ("image",), "conv_direct_k", ELEMS),
                                                 ("add", "sN", B31, ("sN",), "conv_direct_k", SN)])
# wino_bww.hip
_rows("wino_bww.hip", "wino_bww_k", "wbww", [
    ("in0", "view", B31, ("image",), "bww_lds_k", "plane base z sD is a 32-bit int added to the image's pointer"),
    ("in0", "sN", B31, ("sN",), "bww_lds_k", SN),
    ("in0", "row", B29, ("row",), "bww_lds_k", "LDS-DMA offset inside a plane is a byte offset in a signed 32-bit VGPR (NEW here)"),
    ("dout", "view", B31, ("image",), "bww_lds_k", "stricter than needed: only sN and the image span are used"),
    ("dout", "sN", B31, ("sN",), "bww_lds_k", SN),
    ("dout", "image", B29, ("plane",), "bww_lds_k", BYTES + " inside the image's descriptor"),
])
_rows("wino_bww.hip", "wino_bww_k", "wbww_cat", [
    ("in1", "view", B31, ("image",), "bww_lds_k", "plane base z sD is a 32-bit int added to the image's pointer"),
    ("in1", "sN", B31, ("sN",), "bww_lds_k", SN),
    ("in1", "row", B29, ("row",), "bww_lds_k", "LDS-DMA offset inside a plane is a byte offset in a signed 32-bit VGPR (NEW here)"),
])
# bww_c1.hip
_rows("bww_c1.hip", "bww_c1m_k", "bc1", [
    ("in0", "view", B31, ("image",), "bww_lds_k", "stricter than needed: images are rebased in 64 bits"),
    ("in0", "image", B29, ("plane",), "bww_lds_k", BYTES + " inside the image's descriptor (NEW here: x was unchecked)"),
    ("dout", "view", B31, ("image",), "bww_lds_k", "stricter than needed: images are rebased in 64 bits"),
    ("dout", "image", B29, ("plane",), "bww_lds_k", BYTES + " inside the image's descriptor"),
])
# bww_s2.hip
_rows("bww_s2.hip", "bww_s2_k", "bs2", [
    ("in0", "view", B29, ("image", "plane"), "bww_lds_k", BYTES + " over the whole view"),
    ("dout", "view", B29, ("image",), "bww_lds_k", BYTES + " over the whole view"),
])
# ---- bf16 (2-byte elements; no direct form: past the last bf16 kernel the entry point answers TEM_EUNSUPPORTED)
HB = "byte offset of a buffer load / store: a signed 32-bit VGPR (elements x 2 < 2^31)"
_rows("conv3_bf16.hip", "conv3_bf16_k", "h3", [
    ("in0", "view", B30, ("image", "plane"), "conv_bf16_k", HB),
    ("out0", "view", B30, ("image",), "conv_bf16_k", HB),
])
_rows("conv3_bf16.hip", "conv3_bf16_k", "h3_bd", [("gate", "view", B30, ("image",), None, HB + "; conv_bf16_k has the same limit")])
# (out1 of conv3_bf16_k has no row: it must have out0's strides, so its span passes 2^30 only together with out0's)
_rows("conv3_bf16.hip", "conv3_bf16_k", "h3_cat", [("in1", "view", B30, ("image",), "conv_bf16_k", HB)])
_rows("conv3_bf16.hip", "conv3_bf16_k", "h3_add", [("add", "view", B30, ("image",), None, HB + "; conv_bf16_k has the same limit")])
_rows("conv_bf16.hip", "conv_bf16_k", "h3_cat", [("in1", "view", B31, ("image",), None, ELEMS)])
_rows("conv_bf16.hip", "conv_bf16_k", "h3_split", [("out1", "view", B31, ("image",), None, ELEMS)])
_rows("conv_bf16.hip", "conv_bf16_k", "h1", [
    ("in0", "view", B31, ("image",), None, ELEMS),
    ("out0", "view", B31, ("image",), None, ELEMS),
    ("gate", "view", B30, ("image",), None, HB),
    ("add", "view", B30, ("image",), None, HB),
])
_rows("conv_bf16.hip", "conv_bf16_k", "h1_keep", [
    ("keep", "keep", B33, ("frame",), None, "the keep mask's byte offset (elements / 8) is a signed 32-bit VGPR with the descriptor range an int"),
])
_rows("conv2d_bf16.hip", "conv2d_bf16_k", "h2d", [
    ("in0", "view", B31, ("image", "plane"), None, ELEMS),
    ("out0", "view", B31, ("image",), None, ELEMS),
])
# the epilogue the bf16 kernels share (bf16_common.h: fill_epilogue): gate and add below 2^30 elements; its fits32 test of
# the same views (2^31) lies behind that and has no row
_rows("conv2d_bf16.hip", "conv2d_bf16_k", "h2d_cat", [("in1", "view", B31, ("image",), None, ELEMS)])
_rows("conv2d_bf16.hip", "conv2d_bf16_k", "h2d_split", [("out1", "view", B31, ("image",), None, ELEMS)])
_rows("conv2d_bf16.hip", "conv2d_bf16_k", "h2d_ep", [("gate", "view", B30, ("image",), None, HB),
                                                      ("add", "view", B30, ("image",), None, HB)])
_rows("convT_bf16.hip", "convT_bf16_k", "hT_ep", [("gate", "view", B30, ("image",), None, HB),
                                                   ("add", "view", B30, ("image",), None, HB)])
_rows("convT2d_bf16.hip", "convT2d_bf16_k", "hT2d_ep", [("gate", "view", B30, ("image",), None, HB),
                                                         ("add", "view", B30, ("image",), None, HB)])
_rows("convT_bf16.hip", "convT_bf16_k", "hT", [
    ("in0", "view", B31, ("image",), None, ELEMS),
    ("out0", "view", B31, ("image",), None, ELEMS),
])
_rows("convT2d_bf16.hip", "convT2d_bf16_k", "hT2d", [
    ("in0", "view", B31, ("image",), None, ELEMS),
    ("out0", "view", B31, ("image",), None, ELEMS),
])
_rows("stencil_c1.hip", "c1_mfma_h_k", "hc1m", [
    ("in0", "view", B30, ("image",), "conv_bf16_k", HB + " over the whole view"),
    ("out0", "image", B30, ("plane",), "conv_bf16_k", HB + " inside the image's descriptor"),
])
_rows("stencil_c1.hip", "c1_mfma_h_k", "hc1m_g", [
    ("gate", "image", B30, ("plane",), None, HB + " inside the image's descriptor; conv_bf16_k has the same limit on the view"),
    ("gate", "view", B31, ("image",), None, "stricter than needed: images are rebased in 64 bits; conv_bf16_k stops at 2^30"),
])
_rows("c1out_mfma.hip", "c1out_h_k", "hc1out_g", [
    ("gate", "view", B29, ("image",), None,
     "stricter than needed: shares fits29 with the fp32 kernel, 2^30 would do (conv_bf16_k gates no one-channel output)"),
])
_rows("c1out_mfma.hip", "c1out_h_k", "hc1out", [
    ("in0", "view", B29, ("image",), "conv_bf16_k",
     "a plane of the zero padding adds 2^30 bytes to a valid offset (pd > 0): the view stays below 2^30 bytes, 2^29 bf16 "
     "elements; stricter than needed only for an unpadded launch, where 2^30 elements would do"),
    ("out0", "view", B29, ("image",), "conv_bf16_k", "stricter than needed: shares fits29 with the fp32 kernel, 2^30 would do"),
])
_rows("bww_bf16.hip", "bww_bf16_k", "hbww", [
    ("in0", "view", B31, ("image",), None, ELEMS),
    ("dout", "view", B31, ("image",), None, ELEMS),
])
_rows("bww_bf16.hip", "bww_bf16_k", "hbww_cat", [("in1", "view", B31, ("image",), None, ELEMS)])
_rows("bww2d_bf16.hip", "bww2d_bf16_k", "hbww2d_cat", [("in1", "view", B31, ("image",), None, ELEMS)])
_rows("bww2d_bf16.hip", "bww2d_bf16_k", "hbww2d", [
    ("in0", "view", B31, ("image",), None, ELEMS),
    ("dout", "view", B31, ("image",), None, ELEMS),
])
_rows("bww_c1.hip", "bww_c1m_h_k", "hbc1", [
    ("in0", "view", B30, ("image",), "bww_bf16_k", HB + " inside the image's descriptor; the check is on the view"),
    ("dout", "view", B30, ("image",), "bww_bf16_k", HB + " inside the image's descriptor; the check is on the view"),
])

# the kernels of every family, and the (kernel, operand, quantity) each guards: a thinned LIMITS fails the coverage test
FAMILIES = {
    "conv_s2.hip": ["conv_s2_k"], "c1out_mfma.hip": ["c1out_mfma_k", "c1out_h_k"], "wino.hip": ["wino_conv_k"],
    "stencil_c1.hip": ["c1_mfma_k", "c1_stencil_k", "c1_mfma_h_k"], "convT_mfma.hip": ["convT_mfma_k"],
    "conv_lds.hip": ["conv_lds_k"], "wino_bww.hip": ["wino_bww_k"], "bww_c1.hip": ["bww_c1m_k", "bww_c1m_h_k"],
    "bww_s2.hip": ["bww_s2_k"], "conv3_bf16.hip": ["conv3_bf16_k"], "conv_bf16.hip": ["conv_bf16_k"],
    "conv2d_bf16.hip": ["conv2d_bf16_k"], "convT_bf16.hip": ["convT_bf16_k"], "convT2d_bf16.hip": ["convT2d_bf16_k"],
    "bww_bf16.hip": ["bww_bf16_k"], "bww2d_bf16.hip": ["bww2d_bf16_k"],
}
OPERANDS = {
    "conv_s2.hip": [("conv_s2_k", o, "view") for o in ("in0", "gate", "add", "out0")],
    "c1out_mfma.hip": [("c1out_mfma_k", o, "view") for o in ("in0", "out0", "gate")] +
                      [("c1out_h_k", o, "view") for o in ("in0", "out0", "gate")],
    "wino.hip": [("wino_conv_k", o, q) for o in ("in0", "in1") for q in ("view", "sN", "row")] +
                [("wino_conv_k", o, q) for o in ("out0", "gate") for q in ("view", "sN", "image")] +
                [("wino_conv_k", "out1", "view"), ("wino_conv_k", "out1", "sN"), ("wino_conv_k", "keep", "keep")],
    "stencil_c1.hip": [("c1_mfma_k", "in0", "view"), ("c1_mfma_k", "out0", "image"), ("c1_mfma_k", "out0", "view"),
                       ("c1_mfma_k", "gate", "image"), ("c1_mfma_k", "gate", "view"), ("c1_stencil_k", "in0", "view"),
                       ("c1_stencil_k", "out0", "view"), ("c1_stencil_k", "gate", "view"), ("c1_mfma_h_k", "in0", "view"),
                       ("c1_mfma_h_k", "out0", "image"), ("c1_mfma_h_k", "gate", "image"), ("c1_mfma_h_k", "gate", "view")],
    "convT_mfma.hip": [("convT_mfma_k", o, "view") for o in ("in0", "out0", "gate", "add")] + [("convT_mfma_k", "keep", "keep")],
    "conv_lds.hip": [("conv_lds_k", o, q) for o in ("in0", "in1", "out0", "out1", "gate", "add") for q in ("view", "sN")],
    "wino_bww.hip": [("wino_bww_k", o, q) for o in ("in0", "in1") for q in ("view", "sN", "row")] +
                    [("wino_bww_k", "dout", q) for q in ("view", "sN", "image")],
    "bww_c1.hip": [("bww_c1m_k", o, q) for o in ("in0", "dout") for q in ("view", "image")] +
                  [("bww_c1m_h_k", o, "view") for o in ("in0", "dout")],
    "bww_s2.hip": [("bww_s2_k", o, "view") for o in ("in0", "dout")],
    "conv3_bf16.hip": [("conv3_bf16_k", o, "view") for o in ("in0", "in1", "out0", "gate", "add")],
    "conv_bf16.hip": [("conv_bf16_k", o, "view") for o in ("in0", "in1", "out0", "out1", "gate", "add")] +
                     [("conv_bf16_k", "keep", "keep")],
    "conv2d_bf16.hip": [("conv2d_bf16_k", o, "view") for o in ("in0", "in1", "out0", "out1", "gate", "add")],
    "convT_bf16.hip": [("convT_bf16_k", o, "view") for o in ("in0", "out0", "gate", "add")],
    "convT2d_bf16.hip": [("convT2d_bf16_k", o, "view") for o in ("in0", "out0", "gate", "add")],
    "bww_bf16.hip": [("bww_bf16_k", o, "view") for o in ("in0", "in1", "dout")],
    "bww2d_bf16.hip": [("bww2d_bf16_k", o, "view") for o in ("in0", "in1", "dout")],
}


# ------------------------------------------------------------------------------------------------ building a case
def out_dims(g):
    if g.get("out"):                        # an output view that stops short of the natural extents (plan_cases: odd OD of a transposed layer)
        return g["out"]
    k, s, p = g["k"], g["s"], g["p"]
    f = (lambda d: (d - 1) * s + k - 2 * p) if g["entry"].startswith("convT") else (lambda d: (d + 2 * p - k) // s + 1)
    D, H, W = g["dims"]
    return (f(D) if g["is3d"] else 1, f(H), f(W))


def extents(g):
    """operand -> (D, H, W, C) of geometry g"""
    di, do = g["dims"], out_dims(g)
    e = {"in0": di + (g["ci"],)}
    if g["ci1"]:
        e["in1"] = di + (g["ci1"],)
    if g["entry"].startswith("bww"):
        e["dout"] = do + (g["co"],)
        return e
    e["out0"] = do + (g["co"],)
    if g["co1"]:
        e["out1"] = do + (g["co1"],)
    if g["gate"]:
        e["gate"] = do + (g["co"],)
    if g["add"]:
        e["add"] = do + (g["co"],)
    return e


def _up(v, g):
    return -(-v // g) * g


def stretch(ext, place, limit, side, grid):
    """-> (View, value, step): the operand of extents ext = (D, H, W, C) with its limited quantity at the largest value
    of the alignment grid below `limit` (side "below") or the smallest at or above it ("at")"""
    D, H, W, Cc = ext
    sW, sH, sD = Cc, W * Cc, H * W * Cc
    bump = grid if side == "at" else 0
    if place == "image":
        inner = (D - 1) * sD + (H - 1) * sH + (W - 1) * sW + Cc
        sN = (limit - 1 - inner) // 2 // grid * grid + bump
        return View(3, D, H, W, Cc, sN, sD, sH, sW), 2 * sN + inner, 2 * grid
    if place == "plane":
        if D > 1:
            rest = (H - 1) * sH + (W - 1) * sW + Cc
            sD = (limit - 1 - rest) // (D - 1) // grid * grid + bump
            value, step = (D - 1) * sD + rest, (D - 1) * grid
        else:
            rest = (W - 1) * sW + Cc
            sH = (limit - 1 - rest) // (H - 1) // grid * grid + bump
            value, step = (H - 1) * sH + rest, (H - 1) * grid
        return View(1, D, H, W, Cc, _up(value, grid), sD, sH, sW), value, step
    if place == "row":                      # rows far apart, the planes interleaved one row-length apart
        rest = (W - 1) * sW + Cc
        sH = (limit - 1 - rest) // (H - 1) // grid * grid + bump
        sD = _up(W * Cc, grid)
        assert D * sD <= sH
        value = (H - 1) * sH + rest
        return View(1, D, H, W, Cc, _up((D - 1) * sD + value, grid), sD, sH, sW), value, (H - 1) * grid
    if place == "sN":
        sN = limit - grid + bump
        return View(1, D, H, W, Cc, sN, sD, sH, sW), sN, grid
    raise ValueError(place)


def dense(ext, N):
    D, H, W, Cc = ext
    return View(N, D, H, W, Cc, D * H * W * Cc, H * W * Cc, W * Cc, Cc)


def span(v):
    return (v.N - 1) * v.sN + (v.D - 1) * v.sD + (v.H - 1) * v.sH + (v.W - 1) * v.sW + v.C


class Case:
    """views: operand -> View; value / step: the limited quantity and the alignment grid's step of it; frame: the
    dropout frame (dD, dH, dW) or None"""

    def __init__(self, row, side):
        g = self.geom = GEOM[row.geom]
        self.row, self.side, self.frame = row, side, None
        grid = 16 // g["esz"]                                   # 16-byte chunks: 4 floats, 8 bf16
        ext = extents(g)
        if row.place == "frame":
            N = 1
            self.views = {o: dense(e, N) for o, e in ext.items()}
            dH = dW = 1024
            per = dH * dW * g["co"]                              # keep bits per frame plane
            dD = row.limit // per - (1 if side == "below" else 0)
            self.frame, self.value, self.step = (dD, dH, dW), dD * per, per
            self.org = tuple(f - o for f, o in zip(self.frame, out_dims(g)))   # the output window ends the frame: the largest indices
            return
        v, self.value, self.step = stretch(ext[row.operand], row.place, row.limit, side, grid)
        self.views = {o: (v if o == row.operand else dense(e, v.N)) for o, e in ext.items()}

    def args(self, ptr, w, keep_mask=0, slabs=0):
        """the argument struct with operand pointers ptr[operand] (integers), kernel pointer w; w_layout is the plain
        one (the caller switches to TEM_W_WINOGRAD)"""
        from transfer_em_amd import _lib
        g = self.geom
        bww = g["entry"].startswith("bww")
        a = _lib.tem_bww_args() if bww else _lib.tem_conv_args()

        def put(dst, o):
            v = self.views[o]
            dst.ptr, dst.N, dst.D, dst.H, dst.W, dst.C = ptr[o], v.N, v.D, v.H, v.W, v.C
            dst.sN, dst.sD, dst.sH, dst.sW = v.sN, v.sD, v.sH, v.sW
        put(a.in0, "in0")
        if g["ci1"]:
            put(a.in1, "in1")
        k3 = lambda v, one: (v, v, v) if g["is3d"] else (one, v, v)
        a.kd, a.kh, a.kw = k3(g["k"], 1)
        a.sd, a.sh, a.sw = k3(g["s"], 1)
        a.pd, a.ph, a.pw = k3(g["p"], 0)
        if bww:
            put(a.dout, "dout")
            a.slabs, a.slab_stride, a.nslab, a.accumulate = slabs, 0, MAX_SLABS, 0
            return a
        put(a.out0, "out0")
        if g["co1"]:
            put(a.out1, "out1")
        a.w, a.w_layout = w, (_lib.TEM_W_FLIP_CO_CI if g["flip"] else _lib.TEM_W_TAP_CI_CO)
        a.ep.slope, a.ep.gate_slope = g["slope"], 0.3
        if g["gate"]:
            put(a.ep.gate, "gate")
        if g["add"]:
            put(a.ep.add, "add")
        if g["keep"]:
            a.ep.dropout, a.ep.seed, a.ep.site, a.ep.step = 1, 42, 3, 7
            a.ep.keep_mask, a.ep.keep_mode = keep_mask or 0x7d0000000000, g["keep"]
            if self.frame:
                a.ep.drop_dims[0], a.ep.drop_dims[1], a.ep.drop_dims[2] = self.frame
                a.ep.drop_org[0], a.ep.drop_org[1], a.ep.drop_org[2] = self.org
        return a


def build(row, side):
    return Case(row, side)


def route(lib, case, a, u=None):
    """(rc, kernel symbol) of the launch hip_ops.conv_launch / bww_launch would build from argument struct `a`, which is
    left as that launch takes it: a Winograd layer (`u`: its Winograd-domain kernel copy) that the library runs in the
    Winograd form keeps a.w = u and TEM_W_WINOGRAD, a kernel gradient gets its slab count.

    Two symbols are not the library's word: tem_conv_is_tiled names no kernel for a transposed convolution it does not tile,
    and tem_bww_is_tiled none for the global-load gradient, so "convT_direct_k<ci, co, 0>" and "bww_mfma_k<>" stand for
    "no tiled kernel took it" -- an assertion on them says that much and no more."""
    from transfer_em_amd import _lib
    g, name = case.geom, C.create_string_buffer(96)
    e = g["entry"]
    if e == "conv":
        if g["wino"]:
            plain, a.w_layout = (a.w, a.w_layout), _lib.TEM_W_WINOGRAD
            if u is not None:
                a.w = u
            if lib.tem_conv_is_tiled(C.byref(a), 0, name, 96) == 1:
                return 0, name.value.decode()
            a.w, a.w_layout = plain
        lib.tem_conv_is_tiled(C.byref(a), 0, name, 96)
        return 0, name.value.decode()
    if e == "convT":
        if lib.tem_conv_is_tiled(C.byref(a), 1, name, 96) == 1:
            return 0, name.value.decode()
        return 0, f"convT_direct_k<{g['ci']}, {g['co']}, 0>"
    if e in ("bww", "bww_wino"):
        a.nslab = MAX_SLABS
        if e == "bww_wino":
            nw = lib.tem_conv_bwd_weight_winograd_nslab(C.byref(a), name, 96)
            if nw > 0:
                a.nslab = nw
                return nw, name.value.decode()
        n = lib.tem_conv_bwd_weight_nslab(C.byref(a))
        if n < 1:
            return n, ""
        a.nslab = n
        tiled = lib.tem_bww_is_tiled(C.byref(a), name, 96) == 1
        return n, name.value.decode() if tiled else "bww_mfma_k<>"
    if e == "bww_h":
        a.nslab = MAX_SLABS
        n = lib.tem_conv_bwd_weight_bf16_nslab(C.byref(a), name, 96)
        if n > 0:
            a.nslab = n
        return n, name.value.decode() if n > 0 else ""
    fn = lib.tem_conv_transpose_bf16_describe if e == "convT_h" else lib.tem_conv_bf16_describe
    rc = fn(C.byref(a), name, 96)
    return rc, name.value.decode() if rc == 0 else ""


def query(lib, row, case):
    """the dry answer on made-up pointers (16-byte aligned, one region per operand)"""
    ptr = {o: 0x7f0000000000 + (i << 40) for i, o in enumerate(("in0", "in1", "out0", "out1", "gate", "add", "dout"))}
    return route(lib, case, case.args(ptr, 0x7e0000000000, slabs=0x40000000))


# ------------------------------------------------------------------------------------------------ sentinel frames
# An operand under test lies inside one allocation with head room before its first element; the whole allocation starts
# as a NaN with a payload no kernel produces.  (torch tensors on any device: the host test breaks a stand-in on the CPU.)
SENTINEL = {4: 0x7FC0DEAD, 2: 0x7FC1}          # fp32 / bf16 bit patterns as int32 / int16


def head_room(view_span, word=1 << 31):
    """elements in front of a stretched view: min(span, 2^31), so that a true in-view offset truncated to 32 bits, element or
    byte, signed or unsigned, still lands inside the allocation (`word`: half the range of the offset register; the host
    test's scale model has a 16-bit one)"""
    return _up(min(view_span, word), 64)


def _bits(buf):
    import torch
    return buf.view(torch.int32 if buf.element_size() == 4 else torch.int16)


def framed(v, dtype, device, head):
    """(allocation filled with the sentinel, the view `v` inside it behind `head` elements)"""
    import torch
    buf = torch.empty(head + span(v) + 64, dtype=dtype, device=device)        # (+ a sentinel tail)
    _bits(buf).fill_(SENTINEL[buf.element_size()])
    return buf, buf.as_strided((v.N, v.D, v.H, v.W, v.C), (v.sN, v.sD, v.sH, v.sW, 1), head)


def frame_intact(buf, view, chunk=1 << 28):
    """-> (the view's values, compact; elements outside the view that no longer hold the sentinel).  The view itself is
    overwritten with the sentinel on the way, so that one pass over the allocation counts the rest."""
    sent = SENTINEL[buf.element_size()]
    inside = view.clone()
    bits = _bits(buf)
    bits.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(sent)
    bad = 0
    for i in range(0, bits.numel(), chunk):
        bad += int((bits[i:i + chunk] != sent).sum())
    return inside, bad
