"""Attention inputs whose logits are EXACT INTEGERS of the size trained non-local blocks produce (no 1 / sqrt(d) in the
reference: |s| of a hundred and more), shared by test_attention_logits_host.py and test_gpu_attention_logits.py.

Large logits make softmax ill-conditioned: a rounding of s by one ulp at |s| = 200 moves a weight by 1e-5, and an honest
tolerance would have to grow with |s|.  Here theta and phi hold only small integers (|v| <= 128: exact in bf16, in fp16,
and with a zero lo half under split operands), and every partial sum of theta . phi stays far below 2^24, so S is the
same integer in fp32, fp16, split-operand, bf16 and fp64 arithmetic in any summation order.  What is left to differ is
the softmax itself -- the running max, the rescale of O, the merges -- and the existing bars of the kernels apply.

Layout of a theta / phi row (d columns):
  column 0      theta = 1,    phi = b_j   the key profile (below)
  column 1      theta = r_i,  phi = 1     a per-query shift r_i = ((i % 7) - 3) * 40: softmax does not see it, a maximum
                                          shared between queries or taken from the wrong lane does
  columns 2..7  sparse noise, theta in {-1, 0, 1}, phi in {-2 .. 2}  (|noise| <= 12; at most d - 2 columns)
  the rest      zero
so s_ij = b_j + r_i + noise_ij, within +-252."""
import torch

PEAK = 96
PROFILES = ("late_peak", "peak_group0", "peak_group1", "ascending", "descending", "low", "high", "uniform")
ONE_HOT = ("late_peak", "peak_group0", "peak_group1")


def row_shift(Nq):
    return ((torch.arange(Nq) % 7) - 3) * 40


def peak_key(profile, Nk, group_keys):
    """The key that carries +PEAK.  late_peak: the last key (the ragged tail tile).  peak_group0 / peak_group1: a key of the
    first / second key group of a key-split tile (a tile = two groups of `group_keys` keys: 16 | 16 for the fp32 8-wave
    kernel, 32 | 32 for the bf16 one), in the middle tile, so that one group carries the maximum and the other merges
    against it from far below.  None: the shape has no such key."""
    if profile == "late_peak":
        return Nk - 1
    if group_keys is None:
        return None
    tile = 2 * group_keys
    j = ((Nk - 1) // tile // 2) * tile + (group_keys if profile == "peak_group1" else 0) + 5
    return j if j < Nk else None


def key_profile(profile, Nk, group_keys=None):
    """b_j, int64 [Nk]."""
    j = torch.arange(Nk)
    if profile in ONE_HOT:
        b = torch.zeros(Nk, dtype=torch.int64)
        b[peak_key(profile, Nk, group_keys)] = PEAK
        return b
    if profile == "ascending":                      # every tile raises the maximum: O is rescaled at every step
        return (120 * j) // Nk
    if profile == "descending":                     # the rescale never fires after tile 0
        return (120 * (Nk - 1 - j)) // Nk
    if profile == "low":                            # underflows without max subtraction
        return torch.full((Nk,), -100, dtype=torch.int64)
    if profile == "high":                           # overflows without it
        return torch.full((Nk,), 100, dtype=torch.int64)
    if profile in ("uniform", "zero"):              # uniform: no noise either, y = mean(g); zero: b = 0 under the noise
        return torch.zeros(Nk, dtype=torch.int64)
    raise ValueError(profile)


def profiles_for(Nk, group_keys):
    return [p for p in PROFILES if p not in ONE_HOT or peak_key(p, Nk, group_keys) is not None]


def make_inputs(profile, B, Nq, Nk, d, dv, group_keys=None, shift=True, seed=0):
    """(theta [B, Nq, d], phi [B, Nk, d], g [B, Nk, dv]) in fp32; theta / phi integer valued, g seeded Gaussian (round it
    to the operand type where that is narrower).  shift=False: r_i = 0, the same noise and the same g."""
    gen = torch.Generator().manual_seed(77000 + 131 * seed + 7 * d + dv + Nk)
    g = torch.randn(B, Nk, dv, generator=gen)
    th = torch.zeros(B, Nq, d)
    ph = torch.zeros(B, Nk, d)
    nn = max(0, min(6, d - 2))
    # drawn whatever the profile, so that every profile of a shape sees the same noise and the same g
    t_noise = torch.randint(-1, 2, (B, Nq, nn), generator=gen).float() * (torch.rand(B, Nq, nn, generator=gen) < 0.5)
    p_noise = torch.randint(-2, 3, (B, Nk, nn), generator=gen).float()
    th[..., 0] = 1.0
    ph[..., 0] = key_profile(profile, Nk, group_keys).float()
    ph[..., 1] = 1.0
    if shift:
        th[..., 1] = row_shift(Nq).float()
    if profile != "uniform":
        th[..., 2:2 + nn] = t_noise
        ph[..., 2:2 + nn] = p_noise
    return th, ph, g


def todays_inputs(B, Nq, Nk, d, dv):
    """The operands tests/test_gpu_kernels.py::test_fused_nonlocal_attention draws (logits of a few units)."""
    gen = torch.Generator().manual_seed(1000 + Nq + d)
    ld = (2 * d + dv + 3) // 4 * 4 + 4
    tpg_q = torch.randn(B, Nq, ld, generator=gen)
    tpg_k = torch.randn(B, Nk, ld, generator=gen)
    return tpg_q[..., :d] * (3.0 / d ** 0.5), tpg_k[..., d:2 * d].clone(), tpg_k[..., 2 * d:2 * d + dv].clone()


def logits(th, ph, dtype=torch.float64):
    return th.to(dtype) @ ph.to(dtype).transpose(1, 2)


def reference(th, ph, g, kind="softmax", dtype=torch.float64):
    """softmax(theta phi^T) g, (theta phi^T / Nk) g or (relu(theta phi^T) / Nk) g in `dtype` on the CPU."""
    s = logits(th, ph, dtype)
    if kind == "softmax":
        p = torch.softmax(s, -1)
    elif kind == "scale":
        p = s / s.shape[-1]
    else:
        p = s.clamp_min(0) / s.shape[-1]
    return p @ g.to(dtype)


def online_softmax_emulation(th, ph, g, tile=16, mutation=None):
    """The kernels' tiled online softmax in fp32 on the CPU: per `tile` keys a running max m, a running sum l and an
    output O rescaled by exp(m_old - m_new).  mutation "shared_max": the 16 queries of a wave share one maximum (what a
    reduction over the wrong axis, or an alpha fetched from the wrong lane, amounts to); "no_max": exp(s) unshifted."""
    th, ph, g = th.float(), ph.float(), g.float()
    S = th @ ph.transpose(1, 2)
    B, Nq, Nk = S.shape
    m = torch.full((B, Nq), float("-inf")) if mutation != "no_max" else torch.zeros(B, Nq)
    l = torch.zeros(B, Nq)
    O = torch.zeros(B, Nq, g.shape[2])
    for k0 in range(0, Nk, tile):
        s = S[:, :, k0:k0 + tile]
        mx = s.max(-1).values
        if mutation == "shared_max":
            pad = (-Nq) % 16
            grp = torch.cat([mx, torch.full((B, pad), float("-inf"))], 1).view(B, -1, 16).max(-1, keepdim=True).values
            mx = grp.expand(-1, -1, 16).reshape(B, -1)[:, :Nq]
        m_new = torch.maximum(m, mx) if mutation != "no_max" else m
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        O = O * alpha[..., None] + p @ g[:, k0:k0 + tile]
        m = m_new
    return O / l[..., None]


def narrow_emulation(th, ph, g, dtype):
    """softmax attention with the operands, P (unnormalised, max 1) and -- for bf16 -- y each rounded ONCE to `dtype`
    (torch.bfloat16: the bf16 kernel's contract; torch.float16: PTX_NL_F16, whose y stays fp32); everything else fp64."""
    rnd = lambda t: t.to(dtype).double()
    s = logits(rnd(th), rnd(ph))
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    y = (rnd(p) @ rnd(g)) / p.sum(-1, keepdim=True)
    return rnd(y) if dtype == torch.bfloat16 else y


# ---------------------------------------------------------------------------------------------------------------- shapes
# One row per kernel the dispatcher at the end of nonlocal_attn.hip can choose (ptx_nonlocal_ws_fwd, in its order of tests):
# (id, flavour, kind, B, Nq, Nk, d, dv, group_keys).  group_keys: keys per key group of a key-split tile, None without one.
FP32_ROWS = [
    # PTX_NL_F16, dv <= 64: launch_nl_mode<64, 64, true, 1>
    ("f16", "f16", "softmax", 2, 100, 50, 32, 40, None),
    # Nq <= 512, 64 < d <= 256, dv <= 256: the d-split kernel launch_nl_ds<256, 256, 4>
    ("dsplit256", "", "softmax", 2, 50, 25, 200, 136, None),
    # Nq <= 512, 256 < d <= 512: launch_nl_ds<512, 512, 8>
    ("dsplit512", "", "softmax", 1, 50, 40, 320, 264, None),
    # d > 512: theta from global, launch_nl_tg<1024, 128>, dv = 320 over three blockIdx.y chunks
    ("theta_global", "", "softmax", 1, 100, 60, 640, 320, None),
    # Nq > 512 (no d-split), 64 < d <= 256, Nk >= 128: key split launch_nl_ks<256, 256>; group g of a 32-key tile takes keys
    # [16 g, 16 g + 16) (k_row_off = (16 * grp + n) * D); the last tile (13 keys) leaves group 1 empty
    ("ksplit", "", "softmax", 1, 530, 333, 200, 200, 16),
    # the same under split operands: launch_nl_ks_x3<256, 128>
    ("ksplit_x3", "x3", "softmax", 2, 520, 160, 96, 128, 16),
    # d <= 64, dv <= 64, fp32: the 64-query tile launch_nl<64, 64>
    ("tile64", "", "softmax", 2, 100, 100, 16, 16, None),
    # d <= 64 under split operands: launch_nl_x3<64, 64>
    ("x3", "x3", "softmax", 2, 90, 90, 40, 24, None),
    # PTX_NL_SCALE on launch_nl<64, 64> / launch_nl_x3<64, 64>, and PTX_NL_SCALE | PTX_NL_RELU on 4-float rows
    ("scale", "", "scale", 2, 90, 90, 40, 24, None),
    ("scale_x3", "x3", "scale", 2, 90, 90, 40, 24, None),
    ("relu", "", "relu", 2, 90, 70, 4, 24, None),
]
# PTX_NL_STREAMK=1 with a workspace: nl_sk_chunks = 32 (9 query tiles), launch_nl_sk<256, 256, 0>.  32 key tiles of 32 keys,
# 288 units, 9 per chunk: every query tile is cut into 4 or 5 pieces, and a single peak key lies in exactly one of them.
STREAMK_ROW = ("streamk", "", "softmax", 1, 530, 1000, 200, 136, 16)
# bf16 (ptx_nonlocal_bf16_variant_fwd), (d, dv, Nq, Nk).  Variant 1 tiles are 64 keys, 32 | 32 (k_row_off = (16 KT grp + n) D)
BF16_ROWS = [
    (256, 256, 70, 97),       # D = 256, DV = 256; Nk = 64 + 33: group 1 owns one key of the last tile
    (32, 256, 37, 65),        # D = 32; Nk = 64 + 1
    (10, 10, 64, 64),         # odd widths, D = 32, DV = 64
    (256, 512, 17, 65),       # dv split over blockIdx.y
    (256, 256, 64, 9),        # variant 1: group 1 sees no key at all (the merge's exp(-inf) path)
]
BF16_BATCH = 3
SOFTMAX_COLS = (37, 196, 1568)                        # softmax_rows_kernel<4>, <4> and <32> (ld <= 256, <= 256, <= 2048)


def softmax_rows_logits(cols):
    """Integer logit rows for ptx_softmax_rows / ptx_views_mean, [rows, cols] fp32: every key profile (SOFTMAX_ROWS) at
    shift 0, then at each of the seven row shifts, all under one +-12 integer noise pattern.  Exact in bf16 too
    (|x| <= 252).  Returns (x, rows per shift block)."""
    gen = torch.Generator().manual_seed(4100 + cols)
    noise = torch.randint(-12, 13, (cols,), generator=gen)
    base = torch.stack([key_profile(p, cols, 16) + (0 if p == "uniform" else noise) for p in SOFTMAX_ROWS])
    shifts = [0] + [(k - 3) * 40 for k in range(7)]
    return torch.cat([base + s for s in shifts]).float(), len(SOFTMAX_ROWS)


SOFTMAX_ROWS = PROFILES + ("zero",)
