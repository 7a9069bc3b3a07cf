#!/usr/bin/env python
"""Fingerprint of the plans the engine compiles, without a GPU: dry plans on the 'meta' device for a fixed list of
(factory, shape, arithmetic), one line per plan with the number of steps, the number of launches a forward runs (the
active side of every chain-or-pair decision), the split-K workspace size and a hash over every step's class name, label,
conv descriptor key(s), tile, split, MACs and HBM bytes (both sides of every chain-or-pair decision and the decision
itself; no pointers).  Two trees built from the same kernels that print the same lines compile the same plans: run it
before and after a change to the host code that must not change what is launched.

    python scripts/plan_fingerprint.py
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pretorched_x_amd as ptx                                   # noqa: E402
from pretorched_x_amd import _lib                                # noqa: E402
from pretorched_x_amd.engine import AltStep, Engine, Plan, _WinoExec       # noqa: E402

CLIP_FULL, CLIP_SMALL = (8, 3, 16, 224, 224), (1, 3, 8, 64, 64)


def _zoo(name, **kw):
    try:
        return ptx.__dict__[name](pretrained=None, **kw)
    except TypeError:
        return ptx.__dict__[name](**kw)


def _nl(dtype):
    return ptx.NonLocalBlock3D(64, mode="embedded_gaussian", sub_sample=True, bn_layer=True).eval().to(dtype)


# (row name, model factory, plan shape, Engine.precision, parameter dtype)
CASES = [
    ("resnet3d50 fp32 cfg2", lambda: _zoo("resnet3d50", num_classes=339), CLIP_FULL, "fp32", None),
    ("resnet3d50 x3 cfg2", lambda: _zoo("resnet3d50", num_classes=339), CLIP_FULL, "x3", None),
    ("resnet3d50 bf16 cfg2", lambda: _zoo("resnet3d50", num_classes=339), CLIP_FULL, "fp32", torch.bfloat16),
    ("r2plus1d18 fp32", lambda: _zoo("r2plus1d18", num_classes=339), CLIP_FULL, "fp32", None),
    ("resnet3d18 fp32 small", lambda: _zoo("resnet3d18", num_classes=339), CLIP_SMALL, "fp32", None),
    ("resnet18 2-D cfg1", lambda: _zoo("resnet18", num_classes=1000), (1, 3, 224, 224), "fp32", None),
    ("nonlocal_r2plus1d50 cfg3", lambda: ptx.nonlocal_r2plus1d50(339), (8, 3, 32, 112, 112), "fp32", None),
    ("nonlocal_r2plus1d50 x3 cfg3", lambda: ptx.nonlocal_r2plus1d50(339), (8, 3, 32, 112, 112), "x3", None),
    ("i3d cfg4", lambda: ptx.i3d(400), (2, 3, 64, 224, 224), "fp32", None),
    ("biggan_deep256 fp16 cfg5", lambda: ptx.biggan_deep(256, precision="fp16"), (32, 128), "fp32", None),
    ("biggan_deep256 fp32 cfg5", lambda: ptx.biggan_deep(256, precision="fp32"), (32, 128), "fp32", None),
    ("biggan_deep256 bf16", lambda: ptx.biggan_deep(256), (32, 128), "fp32", torch.bfloat16),
    ("slowfast50 SF", lambda: ptx.slowfast.resnet50(num_classes=7), (2, 3, 64, 224, 224), "fp32", None),
    ("slowfast18 SF small", lambda: ptx.slowfast.resnet18(mode="SF", num_classes=3), (1, 3, 32, 64, 64), "fp32", None),
    ("trn backbone resnet50", lambda: ptx.TRN(10, num_segments=8, arch="resnet50", pretrained=None).base_model,
     (16, 3, 224, 224), "fp32", None),
    ("nonlocalresnet3d50", lambda: _zoo("nonlocalresnet3d50"), (1, 3, 16, 224, 224), "fp32", None),
    ("resnext3d50 small", lambda: ptx.resnext3d50(num_classes=10), CLIP_SMALL, "fp32", None),
    ("nlblock3d fp32", lambda: _nl(torch.float32), (2, 64, 4, 8, 8), "fp32", None),
    ("nlblock3d bf16", lambda: _nl(torch.bfloat16), (2, 64, 4, 8, 8), "fp32", None),
    ("mnist_nl bf16", lambda: ptx.MNISTNonLocalNet().eval().to(torch.bfloat16), (2, 1, 28, 28), "fp32", None),
]


def _desc(step, name):
    d = getattr(step, name, None)
    return None if d is None else list(d.key())


def _record(step):
    """What a step is, without pointers: attributes missing on a step class read as None."""
    rec = [type(step).__name__, getattr(step, "label", None), _desc(step, "d"), _desc(step, "d2"),
           getattr(step, "cfg", None), getattr(step, "split", None),
           getattr(step, "macs", None), getattr(step, "hbm_bytes", None)]
    if isinstance(step, AltStep):
        rec += [bool(step.use_chain), _record(step.chain), [_record(s) for s in step.pair]]
    if isinstance(step, _WinoExec):
        rec += [bool(step.use_wino), [_record(s) for s in step.direct], [_record(s) for s in step.wino or []],
                bool(step.use_wino4), [_record(s) for s in step.wino4 or []]]
    return rec


def fingerprint(plan):
    blob = json.dumps([_record(s) for s in plan.steps], sort_keys=True).encode()
    launches = sum(len(s.active()) if isinstance(s, (AltStep, _WinoExec)) else 1 for s in plan.steps)
    return len(plan.steps), launches, int(plan.ws_bytes), hashlib.sha256(blob).hexdigest()[:16]


def main():
    print("library %s, %d conv tile configs" % (_lib.binary_source_hash()[:16], _lib.lib().ptx_conv3d_num_configs()))
    rows = []
    for name, make, shape, precision, dtype in CASES:
        model = make().eval()
        if dtype is not None:
            model = model.to(dtype)
        eng = Engine()
        eng.precision = precision
        rows.append((name, eng.dry_plan(model, shape)))
    # decoded uint8 frames (Engine.forward_frames): the plan carries a NormDesc and starts with the normalising pass
    m = _zoo("resnet3d18", num_classes=10).eval()
    norm = _lib.NormDesc.make([0.4, 0.4, 0.4], [0.2, 0.2, 0.2], "RGB", [0, 1])
    rows.append(("resnet3d18 uint8 frames", Plan(m.engine(), m, (2, 3, 8, 64, 64), torch.device("meta"), norm)))
    for name, plan in rows:
        print("%-30s steps %3d  launches %3d  ws_bytes %10d  %s" % ((name,) + fingerprint(plan)))


if __name__ == "__main__":
    main()
