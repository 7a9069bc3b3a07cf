"""Host tests (no GPU) of BatchMix (`pretorched.transforms.BatchMix`, include/ptx_amd_mix.h): the draw against an independent
restatement of torchvision's RandomErasing.get_params loop and v2's MixUp / CutMix draw, the Dirichlet draw against Beta's, the
torch statement of the arithmetic against the naive tensor expressions, the soft targets, argument and row errors (Python and the
library's own host check), the C ABI, and the place of the mix draw behind every other draw of a transform."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 32, 32])
NAMES = ["ptx_batch_mix_apply", "ptx_batch_mix_supported", "ptx_batch_mix_targets"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------- the draw
def erase_get_params(H, W, p, scale, ratio, g):
    """torchvision.transforms.RandomErasing: forward's coin, then get_params' loop on an H x W image."""
    if not torch.rand(1, generator=g) < p:
        return [0, 0, 0, 0, 0]
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(), generator=g)).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < H and w < W):
            continue
        i = torch.randint(0, H - h + 1, size=(1,), generator=g).item()
        j = torch.randint(0, W - w + 1, size=(1,), generator=g).item()
        return [1, i, j, h, w]
    return [0, 0, 0, 0, 0]


def mix_make_params(H, W, mixup_alpha, cutmix_alpha, prob, switch_prob, g):
    """(mode, lam, box): the coin, the switch, torchvision v2's lam and (CutMix.make_params) its box."""
    if mixup_alpha <= 0 and cutmix_alpha <= 0:
        return 0, 1.0, [0, 0, 0, 0]
    if not torch.rand(1, generator=g) < prob:
        return 0, 1.0, [0, 0, 0, 0]
    cut = cutmix_alpha > 0
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut = bool(torch.rand(1, generator=g) < switch_prob)
    alpha = cutmix_alpha if cut else mixup_alpha
    lam = float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), g)[0, 0])
    if not cut:
        return 1, lam, [0, 0, 0, 0]
    r_x = torch.randint(W, size=(1,), generator=g)
    r_y = torch.randint(H, size=(1,), generator=g)
    r = 0.5 * math.sqrt(1.0 - lam)
    r_w_half, r_h_half = int(r * W), int(r * H)
    x1, y1 = int(torch.clamp(r_x - r_w_half, min=0)), int(torch.clamp(r_y - r_h_half, min=0))
    x2, y2 = int(torch.clamp(r_x + r_w_half, max=W)), int(torch.clamp(r_y + r_h_half, max=H))
    return 2, float(1.0 - (x2 - x1) * (y2 - y1) / (W * H)), [y1, x1, y2, x2]


def restated_draw(N, H, W, g, mode, mixup_alpha, cutmix_alpha, prob=1.0, switch_prob=0.5, erase_prob=0.25, scale=(0.02, 0.33),
                  ratio=(0.3, 3.3)):
    rows, lam = np.zeros((N, 11), np.int64), np.ones(N)
    for i in range(N):
        rows[i, 0] = i
        rows[i, 6:11] = erase_get_params(H, W, erase_prob, scale, ratio, g)
    shared = mix_make_params(H, W, mixup_alpha, cutmix_alpha, prob, switch_prob, g) if mode == "batch" else None
    for i in range(N):
        m, l, box = shared if shared is not None else mix_make_params(H, W, mixup_alpha, cutmix_alpha, prob, switch_prob, g)
        if m:
            rows[i, 0], rows[i, 1], lam[i] = (i - 1) % N, m, l
            rows[i, 2:6] = box
    return rows, lam


@pytest.mark.parametrize("mode", ["batch", "clip"])
@pytest.mark.parametrize("alphas", [(0.8, 0.0), (0.0, 1.0), (0.8, 1.0)], ids=["mixup", "cutmix", "both"])
def test_draw_equals_the_restated_order(ptx, mode, alphas):
    TF = ptx.transforms
    kinds = set()
    for seed in range(20):
        kw = dict(prob=0.8, switch_prob=0.4, erase_prob=0.6)
        bm = TF.BatchMix(alphas[0], alphas[1], mode=mode, generator=gen(seed), **kw)
        rows, lam = bm.draw(5, 24, 36)
        want_rows, want_lam = restated_draw(5, 24, 36, gen(seed), mode, alphas[0], alphas[1], **kw)
        assert rows.dtype == torch.int32 and lam.dtype == torch.float64
        assert np.array_equal(rows.numpy(), want_rows) and np.array_equal(lam.numpy(), want_lam), seed
        kinds |= set(rows[:, 1].tolist())
        bm.check_params((rows, lam), 5, 24, 36)
        mixed = rows[:, 1] != 0
        assert torch.equal(rows[mixed, 0], (torch.arange(5, dtype=torch.int32)[mixed] - 1) % 5)
        assert bool(((rows[:, 9] < 24) & (rows[:, 10] < 36)).all())
    assert kinds == {0} | ({1} if alphas[0] else set()) | ({2} if alphas[1] else set())


def test_zero_probabilities_give_empty_rows(ptx):
    TF = ptx.transforms
    rows, lam = TF.BatchMix(erase_prob=0.0, prob=0.0, generator=gen(3)).draw(4, 16, 20)
    assert torch.equal(rows[:, 0], torch.arange(4, dtype=torch.int32)) and not rows[:, 1:].any() and torch.equal(lam, torch.ones(4, dtype=torch.float64))
    rows, lam = TF.BatchMix(0.0, 0.0, erase_prob=0.0, generator=gen(3)).draw(4, 16, 20)
    assert not rows[:, 1:].any()
    x = torch.randn(4, 3, 2, 16, 20)
    assert torch.equal(TF.batch_mix_torch(x, (rows, lam)), x)
    # an unmixed draw consumes the coins alone: the erase coin per clip, then the mix coin
    g1, g2 = gen(9), gen(9)
    TF.BatchMix(erase_prob=0.0, prob=0.0, generator=g1).draw(3, 16, 20)
    torch.rand(4, generator=g2)
    assert torch.equal(torch.rand(1, generator=g1), torch.rand(1, generator=g2))


@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0, 4.0])
def test_sample_dirichlet_with_a_generator_equals_beta(alpha):
    for seed in range(10):
        lam = float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), gen(seed))[0, 0])
        torch.manual_seed(seed)
        assert lam == float(torch.distributions.Beta(alpha, alpha).sample(()))


# --------------------------------------------------------------------------------------------- the arithmetic
def hand_rows(N):
    """Rows of every kind on 9 x 13 frames: MixUp with an erased partner, CutMix whose box is straddled by both erases, unmixed."""
    rows = np.zeros((N, 11), np.int64)
    rows[:, 0] = (np.arange(N) - 1) % N
    lam = np.ones(N)
    rows[0, 1], lam[0] = 1, 0.3
    rows[0, 6:11] = 1, 2, 3, 4, 5
    if N > 1:
        rows[1, 1], lam[1] = 2, 0.5
        rows[1, 2:6] = 1, 2, 7, 9
        rows[1, 6:11] = 1, 0, 0, 3, 4
    if N > 2:
        rows[2, 0] = 2
    return rows, lam


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_mix_torch_equals_the_naive_expressions(ptx, dtype):
    TF = ptx.transforms
    x = torch.randn(3, 3, 2, 9, 13, generator=gen(1)).to(dtype)
    value = (0.25, -1.5, 3.0)
    rows, lam = hand_rows(3)
    got = TF.batch_mix_torch(x, (rows, lam), value)
    fill = torch.tensor(value).to(dtype).view(3, 1, 1, 1)
    e = x.clone()
    e[0, :, :, 2:6, 3:8] = fill
    e[1, :, :, 0:3, 0:4] = fill
    assert torch.equal(got[0], e[2].mul(1.0 - 0.3).add_(e[0].mul(0.3)))
    want1 = e[1].clone()
    want1[:, :, 1:7, 2:9] = e[0][:, :, 1:7, 2:9]
    assert torch.equal(got[1], want1) and torch.equal(got[2], x[2]) and got.dtype == dtype
    # a whole batch of MixUp under the cyclic partner is the one-line recipe; noise fills come from the list, in clip order
    rows = np.zeros((3, 11), np.int64)
    rows[:, 0], rows[:, 1] = (np.arange(3) - 1) % 3, 1
    lam = np.full(3, 0.7231)
    assert torch.equal(TF.batch_mix_torch(x, (rows, lam)), x.roll(1, 0).mul(1.0 - 0.7231).add_(x.mul(0.7231)))
    rows[:, 1] = 0
    rows[1, 6:11] = 1, 1, 1, 2, 3
    rows[2, 6:11] = 1, 0, 5, 9, 8
    noise = [torch.randn(3, 2, 2, 3), torch.randn(3, 2, 9, 8)]
    want = x.clone()
    want[1, :, :, 1:3, 1:4] = noise[0].to(dtype)
    want[2, :, :, 0:9, 5:13] = noise[1].to(dtype)
    assert torch.equal(TF.batch_mix_torch(x, (rows, lam), "random", noise), want)


def test_targets(ptx):
    TF = ptx.transforms
    labels = torch.tensor([3, 0, 6, 3])
    for lam_v, smoothing in ((0.3, 0.1), (0.91, 0.0), (0.0, 0.1), (1.0, 0.25)):
        rows = np.zeros((4, 11), np.int64)
        rows[:, 0], rows[:, 1] = (np.arange(4) - 1) % 4, 1
        got = TF.batch_mix_targets_torch(labels, 7, (rows, np.full(4, lam_v)), smoothing)
        off = smoothing / 7
        onehot = torch.full((4, 7), off, dtype=torch.float32)
        onehot[torch.arange(4), labels] = 1.0 - smoothing + off
        assert torch.equal(got, onehot.roll(1, 0).mul(1.0 - lam_v).add_(onehot.mul(lam_v)))
        assert got.dtype == torch.float32 and float((got.sum(1) - 1.0).abs().max()) <= 1e-6
    rows[2] = 0
    rows[2, 0] = 2                                          # an unmixed clip keeps its own row
    got = TF.batch_mix_targets_torch(labels, 7, (rows, np.array([0.4, 0.4, 1.0, 0.4])), 0.1)
    assert torch.equal(got[2], onehot[2] * 0 + torch.where(torch.arange(7) == 6, torch.tensor(1.0 - 0.1 + 0.1 / 7), torch.tensor(0.1 / 7)).float())


# --------------------------------------------------------------------------------------------- errors
def test_argument_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    for kw, what in ((dict(mixup_alpha=-1), "mixup_alpha must be"), (dict(cutmix_alpha=float("nan")), "cutmix_alpha must be"),
                     (dict(prob=1.5), "prob must be a probability"), (dict(switch_prob=-0.1), "switch_prob must be"),
                     (dict(erase_prob="x"), "erase_prob must be"), (dict(mode="pair"), "mode must be 'batch' or 'clip'"),
                     (dict(erase_scale=(0.5, 0.1)), "erase_scale must be"), (dict(erase_ratio=(0.0, 1.0)), "erase_ratio must be"),
                     (dict(erase_value="noise"), "erase_value must be"), (dict(erase_value=(1, 2)), "erase_value must be"),
                     (dict(generator=7), "generator must be a torch.Generator"), (dict(noise_generator=7), "noise_generator must be")):
        with pytest.raises(E, match=what):
            TF.BatchMix(**kw)
    bm = TF.BatchMix()
    with pytest.raises(E, match="no CPU fallback"):
        bm(torch.zeros(2, 3, 2, 8, 8))
    with pytest.raises(E, match="need opts="):
        bm(torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(E, match=r"must be \[N,3,T,H,W\]"):
        bm(torch.zeros(2, 4, 2, 8, 8))
    with pytest.raises(E, match="needs a draw"):
        bm.targets(torch.zeros(2, dtype=torch.int64), 5)
    with pytest.raises(E, match="mix= needs out='tensor'"):
        TF.TransformFrames(OPTS, mix=bm, out="frames")
    with pytest.raises(E, match="mix= needs out='tensor'"):
        TF.SampleClips(OPTS, 4, mix=bm, out="frames")
    with pytest.raises(E, match="mix must be a pretorched.transforms.BatchMix"):
        TF.TransformFrames(OPTS, mix=object())
    with pytest.raises(E, match="mix_params= needs a transform built with mix="):
        TF.TransformFrames(OPTS)(torch.zeros(1, 40, 40, 3, dtype=torch.uint8), mix_params=bm.draw(1, 32, 32))
    with pytest.raises(E, match="mix_params= needs a sampler built with mix="):
        TF.SampleClips(OPTS, 4)([torch.zeros(8, 40, 40, 3, dtype=torch.uint8)], mix_params=bm.draw(1, 32, 32))
    # a transform with mix= writes a tensor, so forward_frames' transform= hook refuses it as it refuses every out="tensor"
    with pytest.raises(E, match="out='frames'"):
        TF.apply_frames_transform(TF.TransformFrames(OPTS, mix=bm), torch.zeros(1, 40, 40, 3, dtype=torch.uint8))


FAULTS = [  # (column, value, lam, message of check_params / ptx_batch_mix_supported)
    (0, 4, 0.5, "partner 4 out of range 0..3"), (0, -1, 0.5, "partner -1 out of range"), (1, 3, 0.5, "mode code 3 out of range"),
    (1, -1, 0.5, "mode code -1 out of range"), (2, -1, 0.5, "box .* negative extent or leaves"), (4, 10, 0.5, "box .* leaves the 9x13 frame"),
    (5, 14, 0.5, "box .* leaves the 9x13 frame"), (3, 12, 0.5, "box .* negative extent"), (7, -1, 0.5, "erase rectangle .* negative extent"),
    (9, -2, 0.5, "erase rectangle .* negative extent"), (9, 8, 0.5, "erase rectangle at \\(2, 3\\) .* leaves the 9x13 frame"),
    (10, 11, 0.5, "erase rectangle .* leaves the 9x13 frame"), (None, None, float("nan"), "lam = nan must be finite"),
    (None, None, float("inf"), "lam = inf must be finite"), (None, None, 1.25, "lam = 1.25 must be finite and in"),
    (None, None, -0.01, "must be finite and in"), (6, 2, 0.5, "erase flag must be 0 or 1"),
]


def base_rows():
    rows = np.zeros((4, 11), np.int64)
    rows[:, 0], rows[:, 1] = (np.arange(4) - 1) % 4, 2
    rows[:, 2:6] = 1, 2, 7, 9
    rows[:, 6:11] = 1, 2, 3, 4, 5
    return rows, np.full(4, 0.5)


@pytest.mark.parametrize("col,val,lam_v,what", FAULTS)
def test_check_params_rejects_each_fault(ptx, col, val, lam_v, what):
    TF, E = ptx.transforms, ptx._lib.PtxError
    bm = TF.BatchMix()
    rows, lam = base_rows()
    bm.check_params((rows, lam), 4, 9, 13)
    if col is not None:
        rows[2, col] = val
    lam[2] = lam_v
    with pytest.raises(E, match=what):
        bm.check_params((rows, lam), 4, 9, 13)
    with pytest.raises(E):                                  # a replay is refused before a device is touched
        bm(torch.zeros(4, 3, 2, 9, 13), params=(rows, lam))


def test_check_params_shapes_and_the_accepted_edges(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    bm = TF.BatchMix()
    rows, lam = base_rows()
    for p, what in (((rows[:, :10], lam), r"rows must be \[N, 11\]"), ((rows, lam[:3]), r"lam must be \[N\]"), ((rows.astype(float), lam), "must hold integers"),
                    ((rows, lam.astype(int)), "must hold floats"), (rows, "must be a pair"), ((rows[:0], lam[:0]), "empty batch")):
        with pytest.raises(E, match=what):
            bm.check_params(p)
    with pytest.raises(E, match="hold 4 clips, the batch holds N = 5"):
        bm.check_params((rows, lam), 5)
    rows[0, 2:6] = 4, 6, 4, 6                               # an empty box
    rows[1, 2:6] = 0, 0, 9, 13                              # the whole frame
    rows[2, 6:11] = 1, 9, 13, 0, 0                          # an empty erase rectangle at the far corner
    rows[3, 6:11] = 1, 0, 0, 9, 13                          # a whole-frame erase (a replayed row may hold one)
    lam[0], lam[1] = 0.0, 1.0
    r, l = bm.check_params((torch.from_numpy(rows), torch.from_numpy(lam)), 4, 9, 13)
    assert r.dtype == torch.int32 and l.dtype == torch.float64 and np.array_equal(r.numpy(), rows)


def test_rows_layout(ptx):
    L, TF = ptx._lib, ptx.transforms
    rows, lam = base_rows()
    lam[1] = 0.3
    rows[3, 6] = 0
    r, noise = TF.batch_mix_rows((rows, lam), 5, (0.5, -2.0, 1.0))
    assert r.shape == (4, L.PTX_MIX_ROW) and r.dtype == np.int32 and noise == 0
    assert r[1, L.PTX_MIX_W_A] == np.float32(0.3).view(np.int32) and r[1, L.PTX_MIX_W_B] == np.float32(1.0 - 0.3).view(np.int32)
    r6, _ = TF.batch_mix_rows((rows, np.full(4, 0.6000000238418579 - 2.0 ** -26)), 5)   # b is the double difference rounded once
    assert r6[0, L.PTX_MIX_W_B] == np.float32(1.0 - (0.6000000238418579 - 2.0 ** -26)).view(np.int32)
    assert r[:, L.PTX_MIX_W_ERASE_KIND].tolist() == [1, 1, 1, 0]
    assert r[0, L.PTX_MIX_W_CONST:L.PTX_MIX_W_CONST + 3].view(np.float32).tolist() == [0.5, -2.0, 1.0]
    assert r[2, L.PTX_MIX_W_BOX:L.PTX_MIX_W_BOX + 4].tolist() == [1, 2, 7, 9] and r[2, L.PTX_MIX_W_ERASE:L.PTX_MIX_W_ERASE + 4].tolist() == [2, 3, 4, 5]
    r, noise = TF.batch_mix_rows((rows, lam), 5, "random")
    assert noise == 3 * 3 * 5 * 4 * 5 and r[:, L.PTX_MIX_W_ERASE_KIND].tolist() == [2, 2, 2, 0]
    assert r[:, L.PTX_MIX_W_NOISE].tolist() == [0, 300, 600, 0] and not r[:, L.PTX_MIX_W_NOISE + 1].any()


# --------------------------------------------------------------------------------------------- the C ABI
def test_mix_header_bindings_and_exports_agree(ptx):
    """The three calls live in include/ptx_amd_mix.h: that header, _lib.SIGNATURES_MIX and the library's exports name the same
    functions, disjoint from every other table, listed in INTEGRATION.md; the ctypes mirror matches field for field."""
    L = ptx._lib
    text = open(L.MIX_HEADER_PATH).read()
    declared = L.header_symbols(L.MIX_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_MIX) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd_randaug.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_MIX[name][0], list(L.SIGNATURES_MIX[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_MIX[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_mix.h" in integ and all(n in integ for n in declared) and "### 1n." in integ
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    body = re.search(r"typedef struct ptx_mix_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in re.sub(r"int(32|64)_t", "", line).split(",") if n.strip()]
    assert fields == [n for n, _ in L.MixDesc._fields_] and C.sizeof(L.MixDesc) == 32
    assert [t for _, t in L.MixDesc._fields_] == [C.c_int32] * 6 + [C.c_int64]
    for name in ("NONE", "MIXUP", "CUTMIX", "ERASE_NONE", "ERASE_CONST", "ERASE_NOISE", "SRC_U8", "SRC_F32", "SRC_BF16", "W_PARTNER", "W_MODE",
                 "W_A", "W_B", "W_BOX", "W_ERASE", "W_ERASE_KIND", "W_CONST", "W_NOISE", "ROW"):
        assert re.search(r"#define PTX_MIX_%s\s+%d\b" % (name, getattr(L, "PTX_MIX_" + name)), text), name
    assert L.PTX_MIX_ROW == 20 and ptx.transforms.MIX_MODES == ("none", "mixup", "cutmix")
    # the build: both headers are hashed into the version and are dependencies of the object that holds the kernels
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10
    assert "batch_mix.h" in build.HEADERS and any(h.endswith("ptx_amd_mix.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith("batch_mix.h") for p in files) and any(p.endswith("ptx_amd_mix.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()


def c_rows(ptx, rows, lam, T=2, value=0):
    r, noise = ptx.transforms.batch_mix_rows((rows, lam), T, value)
    return np.ascontiguousarray(r), noise


def test_supported_rejects_each_fault_without_a_device(ptx):
    L = ptx._lib
    lib = L.lib()

    def supported(desc, r):
        ok = lib.ptx_batch_mix_supported(C.byref(desc) if desc is not None else None, C.c_void_p(r.ctypes.data) if r is not None else None)
        return ok, lib.ptx_last_error().decode()

    rows, lam = base_rows()
    good, _ = c_rows(ptx, rows, lam)
    desc = L.MixDesc(4, 2, 9, 13, L.PTX_MIX_SRC_U8, L.PTX_RESIZE_OUT_F32, 0)
    assert supported(desc, good)[0] == 1
    assert supported(None, good) == (0, "ptx_batch_mix_supported: null descriptor")
    ok, msg = supported(desc, None)
    assert ok == 0 and "null pointer" in msg
    for field, val, what in (("N", 0, "non-positive extent"), ("T", -1, "non-positive extent"), ("H", 0, "non-positive extent"), ("W", 0, "non-positive extent"),
                             ("src_mode", 3, "src_mode=3 is not"), ("out_mode", L.PTX_RESIZE_OUT_U8, "out_mode=0 must be"),
                             ("noise_elems", -1, "noise_elems=-1 is negative")):
        d = L.MixDesc(4, 2, 9, 13, L.PTX_MIX_SRC_U8, L.PTX_RESIZE_OUT_F32, 0)
        setattr(d, field, val)
        ok, msg = supported(d, good)
        assert ok == 0 and what in msg, (field, msg)
    ok, msg = supported(L.MixDesc(4, 2, 9, 13, L.PTX_MIX_SRC_BF16, L.PTX_RESIZE_OUT_F32, 0), good)
    assert ok == 0 and "writes its own type" in msg
    for col, val, lam_v, what in FAULTS[:-1]:
        rows, lam = base_rows()
        if col is not None:
            rows[2, col] = val
        lam[2] = lam_v
        with np.errstate(invalid="ignore"):
            r, _ = c_rows(ptx, rows, lam)
        ok, msg = supported(desc, r)
        assert ok == 0 and "clip 2" in msg and re.search(what.replace("lam = nan must be finite", "lam weight a = nan").replace(
            "lam = inf must be finite", "lam weight a = inf").replace("lam = 1.25 must be finite and in", "lam weight a = 1.25"), msg), (what, msg)
    bad = good.copy()
    bad[1, L.PTX_MIX_W_ERASE_KIND] = 3
    ok, msg = supported(desc, bad)
    assert ok == 0 and "clip 1: erase kind 3 out of range" in msg
    # noise: the [3][T][h][w] block of every noisy clip lies inside the buffer
    rows, lam = base_rows()
    r, noise = c_rows(ptx, rows, lam, 2, "random")
    assert noise == 4 * 3 * 2 * 4 * 5
    dn = L.MixDesc(4, 2, 9, 13, L.PTX_MIX_SRC_F32, L.PTX_RESIZE_OUT_F32, noise)
    assert supported(dn, r)[0] == 1
    dn.noise_elems = noise - 1
    ok, msg = supported(dn, r)
    assert ok == 0 and "clip 3: the noise block of 120 elements at offset 360 lies beyond the noise buffer (479 elements)" in msg
    dn.noise_elems = noise
    r[0, L.PTX_MIX_W_NOISE + 1] = 1                          # offset 2^32
    ok, msg = supported(dn, r)
    assert ok == 0 and "clip 0" in msg and "beyond the noise buffer" in msg
    r[0, L.PTX_MIX_W_NOISE + 1] = -1                         # a negative offset
    assert supported(dn, r)[0] == 0
    # accepted edges: an empty box, the whole frame, an empty and a whole-frame erase, lam 0 and 1
    rows, lam = base_rows()
    rows[0, 2:6] = 4, 6, 4, 6
    rows[1, 2:6] = 0, 0, 9, 13
    rows[2, 6:11] = 1, 9, 13, 0, 0
    rows[3, 6:11] = 1, 0, 0, 9, 13
    lam[0], lam[1] = 0.0, 1.0
    assert supported(desc, c_rows(ptx, rows, lam)[0])[0] == 1


def test_apply_and_targets_refuse_bad_arguments_before_any_launch(ptx):
    L = ptx._lib
    lib = L.lib()
    P = C.c_void_p(64)                                     # never dereferenced: every call below returns before a launch
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"])
    good = L.MixDesc(4, 2, 9, 13, L.PTX_MIX_SRC_U8, L.PTX_RESIZE_OUT_F32, 0)
    for desc, args, what in ((None, (P, P, None, P, C.byref(norm)), "null descriptor"),
                             (L.MixDesc(0, 2, 9, 13, 0, 1, 0), (P, P, None, P, C.byref(norm)), "non-positive extent"),
                             (L.MixDesc(4, 2, 9, 13, 0, 0, 0), (P, P, None, P, C.byref(norm)), "out_mode=0 must be"),
                             (L.MixDesc(4, 2, 9, 13, 1, 2, 0), (P, P, None, P, None), "writes its own type"),
                             (L.MixDesc(4, 2, 40000, 40000, 0, 1, 0), (P, P, None, P, C.byref(norm)), "exceeds 32-bit indexing"),
                             (good, (None, P, None, P, C.byref(norm)), "null pointer"), (good, (P, None, None, P, C.byref(norm)), "null pointer"),
                             (good, (P, P, None, None, C.byref(norm)), "null pointer"), (good, (P, P, None, P, None), "null norm descriptor"),
                             (L.MixDesc(4, 2, 9, 13, 0, 1, 10), (P, P, None, P, C.byref(norm)), "null pointer"),
                             (good, (P, P, None, C.c_void_p(66), C.byref(norm)), "misaligned output"),
                             (L.MixDesc(4, 2, 9, 13, 2, 2, 0), (C.c_void_p(65), P, None, P, None), "misaligned source")):
        status = lib.ptx_batch_mix_apply(C.byref(desc) if desc is not None else None, *args, None)
        assert status in (1, 2) and what in lib.ptx_last_error().decode(), (what, lib.ptx_last_error().decode())
    for args, what in (((None, P, P, 4, 7), "null pointer"), ((P, P, P, 0, 7), "non-positive extent"), ((P, P, P, 4, 0), "non-positive extent"),
                       ((C.c_void_p(68), P, P, 4, 7), "misaligned pointer")):
        assert lib.ptx_batch_mix_targets(*args, 0.0, 1.0, None) in (1, 2) and what in lib.ptx_last_error().decode()


# --------------------------------------------------------------------------------------------- the stage
def test_mix_draws_come_last_under_a_shared_seed(ptx):
    TF = ptx.transforms
    kw = dict(random_short_side=(32, 48), random_crop=True, random_hflip=True)
    g1, g2 = gen(10), gen(10)
    full = TF.TransformFrames(OPTS, generator=g1, color=TF.ColorJitter(0.4, generator=g1), augment=TF.RandAugment(generator=g1),
                              mix=TF.BatchMix(generator=g1), **kw)
    geo, col, aug = full.draw_geometry(3, 90, 120), full.color.draw(3), full.augment.draw(3, 32, 32)
    mixed = full.mix.draw(3, 32, 32)
    plain = TF.TransformFrames(OPTS, generator=g2, color=TF.ColorJitter(0.4, generator=g2), augment=TF.RandAugment(generator=g2), **kw)
    assert torch.equal(plain.draw_geometry(3, 90, 120), geo) and torch.equal(plain.color.draw(3)[1], col[1])
    assert torch.equal(plain.augment.draw(3, 32, 32)[0], aug[0]) and plain.mix is None
    again = TF.BatchMix(generator=g2).draw(3, 32, 32)
    assert torch.equal(again[0], mixed[0]) and torch.equal(again[1], mixed[1])
    rs = full._resize
    assert rs.out == "frames" and rs.color is None and rs.augment is None and rs.mix is None and rs.generator is full.generator
    only = TF.TransformFrames(OPTS, generator=gen(8), mix=TF.BatchMix(generator=gen(9)), **kw)
    assert torch.equal(only.draw_geometry(4, 90, 120), TF.TransformFrames(OPTS, generator=gen(8), **kw).draw_geometry(4, 90, 120))
    assert only._resize is not None and only._resize.out == "frames" and only.out == "tensor" and TF.TransformFrames(OPTS, **kw)._resize is None
    sc = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), mix=TF.BatchMix(generator=gen(12)), **kw)
    ref = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), **kw)
    a, b = sc.draw([(12, 60, 80), (9, 50, 44)]), ref.draw([(12, 60, 80), (9, 50, 44)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and sc._resize.out == "frames" and sc._resize.mix is None and ref._resize is None
