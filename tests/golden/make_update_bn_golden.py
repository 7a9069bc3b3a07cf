"""Writes tests/golden/update_bn.npz: what torch.optim.swa_utils.update_bn leaves in every BatchNorm of a zoo model, in float64.

    python tests/golden/make_update_bn_golden.py

Runs on the CPU with torch alone.  For every case of CASES: the package's model with synth_state_dict(seed=1234, **recipe),
batches drawn with torch.Generator().manual_seed(7) + torch.randn, torch.optim.swa_utils.update_bn on a .double() copy (for
the reset=False / momentum case: the same train()-mode pass with every BN's momentum set, on the synthetic running
statistics), then the eval-mode float64 logits of the first batch.  Stored as float32 roundings of the float64 results:
`<case>/mean`, `<case>/var` (every BN's buffer in model.modules() order, concatenated), `<case>/tracked`, `<case>/logits`,
and `<case>/spec` (the case's entry of CASES as JSON), so the tests rebuild models and inputs from the file alone.
tests/test_update_bn_host.py regenerates one case and compares it with the file.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "update_bn.npz")
SEED_WEIGHTS, SEED_BATCHES, NUM_CLASSES = 1234, 7, 51

# name -> factory, factory keywords, synth_state_dict recipe, batch shapes, update_bn keywords
CASES = {
    "resnet3d18": dict(model="resnet3d18", kwargs={}, recipe={}, shapes=[(2, 3, 8, 64, 64), (3, 3, 8, 64, 64)], call={}),
    "resnet3d50": dict(model="resnet3d50", kwargs={}, recipe={}, shapes=[(8, 3, 4, 64, 64)] * 2, call={}),
    "r2plus1d18": dict(model="r2plus1d18", kwargs={}, recipe={}, shapes=[(2, 3, 8, 64, 64)] * 2, call={}),
    "preact_resnet3d18_A": dict(model="preact_resnet3d18", kwargs={"shortcut_type": "A"}, recipe={}, shapes=[(3, 3, 5, 50, 70)] * 2, call={}),
    "resnext3d10": dict(model="resnext3d10", kwargs={}, recipe={"last_bn_damp": 2.0}, shapes=[(3, 3, 5, 50, 70)] * 2, call={}),
    "resnet50": dict(model="resnet50", kwargs={}, recipe={"last_bn_damp": 0.7}, shapes=[(4, 3, 96, 64)] * 2, call={}),
    "resnet3d18_momentum": dict(model="resnet3d18", kwargs={}, recipe={}, shapes=[(2, 3, 8, 64, 64), (3, 3, 8, 64, 64)],
                                call={"reset": False, "momentum": 0.1}),
}


def build_model(spec):
    """The case's model (float32, CPU, eval mode) with its synthetic weights and running statistics."""
    import pretorched_x_amd as ptx
    from pretorched_x_amd.testing import synth_state_dict
    factory = getattr(ptx, spec["model"])
    try:
        model = factory(num_classes=NUM_CLASSES, pretrained=None, **spec["kwargs"])
    except TypeError:                    # factories of families without published weights take no `pretrained`
        model = factory(num_classes=NUM_CLASSES, **spec["kwargs"])
    model.load_state_dict(synth_state_dict(model.state_dict(), SEED_WEIGHTS, **spec["recipe"]))
    return model.eval()


def batches(spec):
    g = torch.Generator().manual_seed(SEED_BATCHES)
    return [torch.randn(tuple(s), generator=g) for s in spec["shapes"]]


def bn_layers(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def reference(spec, dtype=torch.float64):
    """(mean, var, tracked, logits) as numpy arrays of `dtype`'s precision: torch's own pass on a copy of the model."""
    model = copy.deepcopy(build_model(spec)).to(dtype)
    xs = [x.to(dtype) for x in batches(spec)]
    call = spec["call"]
    if not call:
        torch.optim.swa_utils.update_bn(xs, model)
    else:                                # update_bn's body without the reset, every BN on the given momentum
        assert call == {"reset": False, "momentum": 0.1}
        keep = {bn: bn.momentum for bn in bn_layers(model)}
        for bn in keep:
            bn.momentum = call["momentum"]
        model.train()
        with torch.no_grad():
            for x in xs:
                model(x)
        for bn, mom in keep.items():
            bn.momentum = mom
    model.eval()
    with torch.no_grad():
        logits = model(xs[0])
    layers = bn_layers(model)
    return (torch.cat([bn.running_mean for bn in layers]).numpy(), torch.cat([bn.running_var for bn in layers]).numpy(),
            np.array([int(bn.num_batches_tracked) for bn in layers], dtype=np.int64), logits.numpy())


def load():
    """{case: dict(spec, mean, var, tracked, logits)} from the committed file."""
    out = {}
    with np.load(PATH) as z:
        for key in z.files:
            case, field = key.split("/")
            out.setdefault(case, {})[field] = z[key]
    for rec in out.values():
        rec["spec"] = json.loads(str(rec["spec"]))
    return out


def main():
    arrays = {}
    for name, spec in CASES.items():
        mean, var, tracked, logits = reference(spec)
        arrays[name + "/mean"], arrays[name + "/var"] = mean.astype(np.float32), var.astype(np.float32)
        arrays[name + "/tracked"], arrays[name + "/logits"] = tracked, logits.astype(np.float32)
        arrays[name + "/spec"] = np.array(json.dumps(spec))
        print("%-22s %3d BNs %6d channels  max|mean| %.3g  max|var| %.3g  max|logit| %.3g" % (
            name, len(tracked), mean.size, np.abs(mean).max(), np.abs(var).max(), np.abs(logits).max()))
    np.savez_compressed(PATH, **arrays)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
