"""The channel-separated networks (ir-CSN / ip-CSN; Tran et al., ICCV 2019) restated with torch.nn.functional, driven from a state
dict alone -- the reference of tests/test_csn_host.py and tests/test_gpu_csn.py.  Nothing of the package is imported: the structure
(blocks per stage, ir / ip, where a shortcut conv sits) is read off the keys, the definition is written out below.

    stem    conv1 (3,7,7) / (1,2,2) / (1,3,3) -> bn1 -> ReLU -> max_pool3d (1,3,3) / (1,2,2) / (0,1,1)
    block   conv1 1x1x1 -> bn1 -> ReLU -> [conv2_pw 1x1x1 -> bn2_pw] -> conv2 3x3x3 DEPTHWISE, stride s, pad 1 -> bn2 -> ReLU
            -> conv3 1x1x1 -> bn3 -> (+ downsample.0 1x1x1 stride s -> downsample.1, or the input) -> ReLU
    stages  stride 1, 2, 2, 2 (all three axes) on the first block of a stage
    head    mean over (T, H, W) -> last_linear
"""
import torch
import torch.nn.functional as F

EPS = 1e-3


def _bn(sd, name, x, training, eps):
    if isinstance(eps, dict):      # {BatchNorm name: eps}; every other BatchNorm has EPS
        eps = eps.get(name, EPS)
    if training:       # batch statistics; the running buffers of the dict are left alone (clones move)
        return F.batch_norm(x, sd[name + ".running_mean"].clone(), sd[name + ".running_var"].clone(), sd[name + ".weight"],
                            sd[name + ".bias"], True, 0.1, eps)
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        False, 0.1, eps)


def layers_of(sd):
    return tuple(len({k.split(".")[1] for k in sd if k.startswith("layer%d." % l)}) for l in (1, 2, 3, 4))


def block(sd, p, x, stride, training=False, eps=EPS):
    out = F.relu(_bn(sd, p + ".bn1", F.conv3d(x, sd[p + ".conv1.weight"]), training, eps))
    if p + ".conv2_pw.weight" in sd:
        out = _bn(sd, p + ".bn2_pw", F.conv3d(out, sd[p + ".conv2_pw.weight"]), training, eps)
    w2 = sd[p + ".conv2.weight"]
    assert w2.shape[1] == 1, "conv2 of a CSN block is depthwise"
    out = F.relu(_bn(sd, p + ".bn2", F.conv3d(out, w2, None, stride, 1, 1, w2.shape[0]), training, eps))
    out = _bn(sd, p + ".bn3", F.conv3d(out, sd[p + ".conv3.weight"]), training, eps)
    if p + ".downsample.0.weight" in sd:
        x = _bn(sd, p + ".downsample.1", F.conv3d(x, sd[p + ".downsample.0.weight"], None, stride), training, eps)
    return F.relu(out + x)


def features(sd, x, training=False, eps=EPS):
    x = F.relu(_bn(sd, "bn1", F.conv3d(x, sd["conv1.weight"], None, (1, 2, 2), (1, 3, 3)), training, eps))
    x = F.max_pool3d(x, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    for li, n in enumerate(layers_of(sd)):
        for bi in range(n):
            x = block(sd, "layer%d.%d" % (li + 1, bi), x, 2 if (li > 0 and bi == 0) else 1, training, eps)
    return x


def logits(sd, feats):
    return F.linear(F.adaptive_avg_pool3d(feats, 1).flatten(1), sd["last_linear.weight"], sd["last_linear.bias"])


def forward(sd, x, training=False, eps=EPS):
    return logits(sd, features(sd, x, training, eps))
