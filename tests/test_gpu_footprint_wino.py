"""Footprint tests of the Winograd executions F(2x2,3x3) and F(4x4,3x3) of stride-1 3x3x3 convs (conv_wino_f32.hip): the input
transform, the grouped GEMM and the output transform, with x, V, M, the transformed filter, the bias, the residual and y (a
channel slice of a wider row) all carved out of one guarded arena (tests/arena.py) at 16 bytes -- "wino_in_f32: pointers must
be 16-byte aligned" and its siblings refuse less -- once under each fill.  Shapes: the padded-pitch / channel-slice cases
of tests/test_gpu_wino.py and tests/test_gpu_wino4.py (Ci = 10 and Co = 18 ragged, ldx = 20 with foreign data past the conv's
channels, ldy = 28), with the same-shape residual of test_conv_wino_f32; tolerance 2e-4 x scale (`close`), as there.
Guards and inputs intact, nothing non-finite in y, pad channels zero, the columns beyond still holding the fill, bit-identical
y under the two fills (no atomics: nothing is excused).  V and M are scratch: the GEMM reads only what the input transform
wrote, the output transform only what the GEMM wrote -- a NaN from the 0xFF fill of either would reach y."""
import ctypes as C

import pytest
import torch

from footprint import DEV, P, ST, cl, judge, r4, repack, rnd, run
from test_gpu_kernels import make_bn, ref_conv
from test_gpu_wino import wino_desc

pytestmark = pytest.mark.gpu

F32 = torch.float32


@pytest.mark.parametrize("kind,W", [("wino", 4), ("wino4", 5)])
def test_wino_three_launches(ptx, kind, W):
    L = ptx._lib
    lib = L.lib()
    fn = lambda name: getattr(lib, name.replace("wino", kind))                       # noqa: E731
    N, Ci, Co, T, H, kT, ldx, ldy = 2, 10, 18, 3, 6, 3, 20, 28
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, 3, 3, seed=2, scale=(2.0 / (Ci * 9 * kT)) ** 0.5)
    bn, res = make_bn(Co, 3), rnd(N, Co, T, H, W, seed=4)
    # the filter: BN fold (ptx_pack_conv_weight), then the Winograd transform -- on plain allocations, back to the host
    pd = L.PackDesc(Co, Ci, kT, 3, 3, r4(Ci), (Co + 127) // 128 * 128, 0)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd = w.contiguous().to(DEV)
    keep = [t.contiguous().to(DEV) for t in bn[:4]]
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), None, *[P(t) for t in keep], C.c_float(bn[4]), P(wp), P(bp), ST()), "pack")
    xd = cl(x, ldx)
    xd[..., Ci:] = 7.0                          # a padded pitch may hold anything past the conv's own channels
    rd = cl(res)
    d = wino_desc(L, N, Ci, Co, T, H, W, kT, ldx, ldy, True, rd.shape[-1])
    assert fn("ptx_conv_wino_f32_supported")(C.byref(d)), lib.ptx_last_error()
    gd = L.ConvDesc()
    L.check(fn("ptx_conv_wino_f32_gemm_desc")(C.byref(d), C.byref(gd)), "gemm desc")
    torch.cuda.synchronize()
    # the Winograd filter transform runs in the arena too; its output is the filter the GEMM below reads
    u = repack(lambda a, b: L.check(fn("ptx_pack_wino_f32_weight")(C.byref(d), a, b, ST()), "pack %s" % kind), wp.cpu(),
               fn("ptx_wino_f32_weight_elems")(C.byref(d)))
    v_elems = gd.N * gd.Ti * gd.Hi * gd.Wi * gd.ldx
    m_elems = gd.N * gd.To * gd.Ho * gd.Wo * gd.ldy
    assert fn("ptx_conv_wino_f32_workspace_bytes")(C.byref(d)) == (4 * v_elems + 255) // 256 * 256 + 4 * m_elems
    want = ref_conv(x.double(), w.double(), (1, 1, 1), (kT // 2, 1, 1), bn=tuple(t.double() for t in bn[:4]) + (bn[4],), relu=True,
                    res=res.double())

    def launch(v, ar):
        L.check(fn("ptx_wino_in_f32")(C.byref(d), P(v["x"]), P(v["V"]), ST()), "%s in" % kind)
        L.check(lib.ptx_conv3d_fwd(C.byref(gd), P(v["V"]), P(v["u"]), None, None, P(v["M"]), None, 0, -1, 1, ST()), "%s gemm" % kind)
        L.check(fn("ptx_wino_out_f32")(C.byref(d), P(v["M"]), P(v["bp"]), P(v["res"]), P(v["y"]), ST()), "%s out" % kind)

    out = run([("x", xd, None, 16, "in"), ("u", u, None, 16, "in"), ("bp", bp.cpu(), None, 16, "in"), ("res", rd, None, 16, "in"),
               ("V", (v_elems,), F32, 16, "scratch"), ("M", (m_elems,), F32, 16, "scratch"), ("y", (N, T, H, W, ldy), F32, 16, "out")],
              launch)
    c4 = r4(Co)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), 2e-4, (Ellipsis, slice(0, Co)), written=(Ellipsis, slice(0, c4)),
          zero=[(Ellipsis, slice(Co, c4))], untouched=[(Ellipsis, slice(c4, ldy))])
