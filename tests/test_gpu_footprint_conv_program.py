"""Footprint test of one conv program (conv_program.hip): the two-bottleneck program of tests/test_conv_program.py::
test_program_every_tile_split_and_grid (2 x 2 x 10 x 10, 256 -> 64 -> 64 -> 256, block 0 strided with its shortcut-B branch as a
second K source, block 1 with an identity residual; six stages) at the library's own tiles and splits.  The input, every packed
filter and bias, every stage's output, the workspace and the device image all sit in one guarded arena (tests/arena.py),
under each fill at identical addresses (the image embeds them, so it is built after the placements).  Alignment: the stage
pointers are ptx_conv3d_fwd's (16 bytes, make_conv_args); the workspace exactly 256 bytes ("conv_program: needs %llu bytes of
256-byte aligned workspace", conv_program.hip:548 -- one less is refused, asserted); the image 16 bytes (it holds pointers).
The workspace is scratch and NOT zeroed: the header says the launch zeroes its control words itself.  Guards and inputs
intact, nothing non-finite in any stage output, pad channels zero, 3e-4 x scale against float64 (that module's `_check`),
bit-identical stage outputs under the two fills (the only atomics are integer counters: nothing is excused)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from arena import FILLS, Arena, arena_bytes, assert_finite, assert_same_bits
from footprint import DEV, P, ST, close64
from test_conv_program import _bottlenecks

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _reference64(net):
    outs = [net.x_cpu.double()]
    for sp in net.specs:
        bn = sp["bn"] if sp["x2"] is None else sp["bn"][0]
        b = [t.double() for t in bn[:4]]
        y = F.batch_norm(F.conv3d(outs[sp["src"]], sp["w"].double(), None, sp["s"], sp["p"]), b[2], b[3], b[0], b[1], False, 0.1, bn[4])
        if sp["x2"] is not None:
            b2, st = sp["bn"][1], sp["x2_stride"]
            c = [t.double() for t in b2[:4]]
            y = y + F.batch_norm(F.conv3d(outs[sp["x2"]], sp["w2"].double(), None, (st, st, st)), c[2], c[3], c[0], c[1], False, 0.1, b2[4])
        if sp["res"] is not None:
            y = y + outs[sp["res"]]
        outs.append(F.relu(y) if sp["relu"] else y)
    return outs


def test_conv_program_in_the_arena(ptx):
    L = ptx._lib
    lib = L.lib()
    net = _bottlenecks(ptx, N=2, T=2, H=10, W=10, planes=64, blocks=2, seed=40)          # packs the filters on plain allocations
    torch.cuda.synchronize()
    want = _reference64(net)
    x_cpu = net.acts[0].cpu()
    packed = [(s["w"].cpu(), s["b"].cpu()) for s in net.stages]
    shapes = [tuple(a.shape) for a in net.acts[1:]]
    # sizes first (a plan needs only the descriptors and non-null pointers: the plain allocations serve)
    info = L.ConvProgramInfo()
    L.check(lib.ptx_conv_program_plan(net.stage_array(), len(net.stages), C.byref(info)), "plan")
    ws_bytes, img_bytes = int(info.workspace_bytes), int(info.image_bytes)
    sizes = ([x_cpu.numel() * 4] + [t.numel() * 4 for w, b in packed for t in (w, b)] + [4 * torch.Size(s).numel() for s in shapes] +
             [ws_bytes, img_bytes])
    guard = max([64 << 10] + sizes)
    ar = Arena(arena_bytes(sizes, guard), DEV, FILLS[0], guard)
    results, addrs = [], None
    for fill in FILLS:
        ar.reset(fill)
        acts = [ar.place(x_cpu, align=16, role="in", name="x")]
        wb = [(ar.place(w, align=16, role="in", name="w%d" % i), ar.place(b, align=16, role="in", name="b%d" % i))
              for i, (w, b) in enumerate(packed)]
        acts += [ar.place(s, F32, align=16, role="out", name="y%d" % i) for i, s in enumerate(shapes)]
        ws = ar.place((ws_bytes // 4,), F32, align=256, role="scratch", name="workspace")
        arr = (L.ConvStage * len(net.stages))()
        for i, s in enumerate(net.stages):
            e = arr[i]
            C.memmove(C.byref(e.desc), C.byref(s["d"]), C.sizeof(L.ConvDesc))
            e.x, e.w_packed, e.bias, e.y = P(acts[s["src"]]), P(wb[i][0]), P(wb[i][1]), P(acts[s["y"]])
            e.x2 = P(acts[s["x2"]]) if s["x2"] is not None else None
            e.res = P(acts[s["res"]]) if s["res"] is not None else None
            e.tile, e.split_k = -1, 0
        host = (C.c_char * img_bytes)()
        st = lib.ptx_conv_program_build(arr, len(arr), P(ws, 32), ws_bytes, host, img_bytes, C.byref(info))        # 128 bytes off
        assert st == 4 and b"256-byte aligned workspace" in lib.ptx_last_error()
        L.check(lib.ptx_conv_program_build(arr, len(arr), P(ws), ws_bytes, host, img_bytes, C.byref(info)), "build")
        image = ar.place(torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).clone(), align=16, role="in", name="image")
        now = [v.data_ptr() for v in acts + [t for p in wb for t in p] + [ws, image]]
        assert addrs is None or addrs == now, "the two fills must run at identical addresses"
        addrs = now
        L.check(lib.ptx_conv_program_fwd(C.byref(info), P(image), P(ws), 2, ST()), "program")
        code = (C.c_int32 * 4)()
        L.check(lib.ptx_conv_program_error(P(ws), code, ST()), "program error word")
        assert code[0] == 0, "program wait expired: %s" % list(code)
        torch.cuda.synchronize()
        outs = ar.check()
        results.append({k: v.detach().cpu().clone() for k, v in outs.items()})
    for i in range(len(net.stages)):
        Co = net.geo[i + 1][4]
        for out, fill in zip(results, FILLS):
            y = out["y%d" % i]
            assert_finite(y, "stage %d (fill 0x%02x)" % (i, fill))
            close64(y[..., :Co], want[i + 1].permute(0, 2, 3, 4, 1), 3e-4, "stage %d (fill 0x%02x)" % (i, fill))
            assert bool((y[..., Co:] == 0).all())
        assert_same_bits(results[0]["y%d" % i], results[1]["y%d" % i], "stage %d" % i)
