"""No-GPU tests of per-clip resize geometry in `pretorched.transforms.TransformFrames` (`random_short_side`,
`random_resized_crop`, `geometry=`): the numpy model (`geometry_tables` + `apply_tables_numpy`) against PIL on the stored cases
(tests/golden/jitter_frames.npz, written by tests/golden/make_jitter_frames_golden.py with PIL only) and on live random boxes,
`draw_geometry` against the literal torch call sequence, `check_geometry` and the constructor's conflicts, and the host-side
checks of the C entry points."""
import ctypes as C
import itertools
import json
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_frames

OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])
S, H, W = 64, 90, 120
RATIO = (3.0 / 4.0, 4.0 / 3.0)


def cases():
    blob = load_golden("jitter_frames")
    return blob, json.loads(str(blob["cases"]))


def test_the_stored_cases_are_what_the_issue_names_and_the_numpy_model_reproduces_them(ptx):
    TF = ptx.transforms
    blob, meta = cases()
    assert [c["name"] for c in meta] == ["mixed_97x131", "tall_600x200", "jitter_90x120", "wide_64x2100"]
    by = {c["name"]: c for c in meta}
    assert by["mixed_97x131"]["T"] == 2 and [0, 0, 97, 131, 80, 108, 16, 44, 1, 0] in by["mixed_97x131"]["geometry"]
    assert [96, 130, 1, 1, 64, 64, 0, 0, 0, 0] in by["mixed_97x131"]["geometry"]
    assert max(t[0] for t in by["tall_600x200"]["taps"]) >= 19 and [1, 7] in by["tall_600x200"]["taps"]
    assert {tuple(g[8:]) for g in by["jitter_90x120"]["geometry"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {tuple(g[4:6]) for g in by["jitter_90x120"]["geometry"]} == {TF.resized_size_for(90, 120, R) for R in (64, 73, 96)}
    assert all(g[1] + min(g[7] * g[3] // g[5], g[3]) >= 2000 for g in by["wide_64x2100"]["geometry"])   # spans start beyond 2048 px
    for c in meta:
        N = len(c["geometry"])
        frames = synth_frames(N * c["T"], c["H"], c["W"], c["seed"]).reshape(N, c["T"], c["H"], c["W"], 3)
        want = blob["out_" + c["name"]]
        assert want.shape == (N, c["T"], S, S, 3)
        for n, row in enumerate(c["geometry"]):
            tables = TF.geometry_tables(row, S)
            assert [tables["rows"][2].shape[1], tables["cols"][2].shape[1]] == c["taps"][n]
            for t in range(c["T"]):
                assert np.array_equal(TF.apply_tables_numpy(frames[n, t], tables), want[n, t]), (c["name"], n, t)


def test_the_numpy_model_equals_pil_on_live_random_boxes(ptx):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    TF = ptx.transforms
    rng = np.random.RandomState(7)
    frames = {(97, 131): synth_frames(1, 97, 131, 1)[0], (600, 200): synth_frames(1, 600, 200, 2)[0]}
    for it in range(50):
        (FH, FW), frame = list(frames.items())[it % 2]
        bh, bw = int(rng.randint(1, FH + 1)), int(rng.randint(1, FW + 1))
        bt, bl = int(rng.randint(0, FH - bh + 1)), int(rng.randint(0, FW - bw + 1))
        h, w = int(rng.randint(S, 100)), int(rng.randint(S, 100))
        if it % 5 == 0:
            h, w = S, S
        top, left = int(rng.randint(0, h - S + 1)), int(rng.randint(0, w - S + 1))
        hf, vf = int(rng.randint(2)), int(rng.randint(2))
        row = [bt, bl, bh, bw, h, w, top, left, hf, vf]
        img = Image.fromarray(frame).crop((bl, bt, bl + bw, bt + bh))
        if (h, w) != (bh, bw):
            img = img.resize((w, h), Image.BILINEAR)
        img = img.crop((left, top, left + S, top + S))
        img = ImageOps.mirror(img) if hf else img
        img = ImageOps.flip(img) if vf else img
        assert np.array_equal(TF.apply_tables_numpy(frame, TF.geometry_tables(row, S)), np.asarray(img)), row


def test_resized_size_for(ptx):
    TF = ptx.transforms
    assert TF.resized_size_for(90, 120, 73) == (73, 97) == TF.resized_size(90, 120, [3, 64, 64])
    assert TF.resized_size_for(120, 90, 73) == (97, 73)
    assert TF.resized_size_for(90, 120, 90) == (90, 120) and TF.resized_size_for(120, 90, 90) == (120, 90)   # not resampled
    assert TF.resized_size_for(90, 120, 64) == (64, 85) and TF.resized_size_for(100, 100, 70) == (70, 70)
    for Hh, Ww in ((90, 120), (120, 90), (64, 2100), (73, 73)):
        for scale in (0.875, 1.0, 0.5):
            assert TF.resized_size(Hh, Ww, [3, 64, 64], scale) == TF.resized_size_for(Hh, Ww, int(math.floor(64 / scale)))


def literal_box(Hh, Ww, scale, ratio, g):
    """torchvision's RandomResizedCrop.get_params, call by call."""
    area = Hh * Ww
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= Ww and 0 < h <= Hh:
            i = torch.randint(0, Hh - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, Ww - w + 1, size=(1,), generator=g).item()
            return i, j, h, w
    in_ratio = float(Ww) / float(Hh)
    if in_ratio < min(ratio):
        w = Ww
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = Hh
        w = int(round(h * max(ratio)))
    else:
        w, h = Ww, Hh
    return (Hh - h) // 2, (Ww - w) // 2, h, w


def literal_geometry(ptx, N, Hh, Ww, g, mode, rc, rh, rv, rrc=None):
    """The contract, call by call: per clip [R] or [get_params], [top, left], [hflip], [vflip] for the switches that are on."""
    TF = ptx.transforms
    out = []
    for _ in range(N):
        box = (0, 0, Hh, Ww)
        if mode == "short_side":
            h, w = TF.resized_size_for(Hh, Ww, int(torch.randint(64, 96 + 1, (1,), generator=g)))
        elif mode == "rrc":
            box = literal_box(Hh, Ww, rrc["scale"], rrc["ratio"], g)
            h, w = S, S
        else:
            h, w = TF.resized_size(Hh, Ww, OPTS["input_size"])
        top, left = int(round((h - S) / 2.0)), int(round((w - S) / 2.0))
        hf = vf = 0
        if rc:
            top = int(torch.randint(0, h - S + 1, (1,), generator=g))
            left = int(torch.randint(0, w - S + 1, (1,), generator=g))
        if rh:
            hf = int(torch.rand(1, generator=g) < 0.5)
        if rv:
            vf = int(torch.rand(1, generator=g) < 0.5)
        out.append(list(box) + [h, w, top, left, hf, vf])
    return torch.tensor(out, dtype=torch.int32)


COMBOS = [(m, rc, rh, rv) for m in ("plain", "short_side", "rrc") for rc, rh, rv in itertools.product((False, True), repeat=3)
          if not (m == "rrc" and rc)]


@pytest.mark.parametrize("mode,rc,rh,rv", COMBOS)
def test_draw_geometry_is_the_literal_torch_sequence(ptx, mode, rc, rh, rv):
    TF = ptx.transforms
    rrc = dict(scale=(0.08, 1.0), ratio=RATIO)
    kw = dict(random_crop=rc, random_hflip=rh, random_vflip=rv)
    if mode == "short_side":
        kw["random_short_side"] = (64, 96)
    elif mode == "rrc":
        kw["random_resized_crop"] = True
    tf = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(11), **kw)
    got = tf.draw_geometry(16, H, W)
    want = literal_geometry(ptx, 16, H, W, torch.Generator().manual_seed(11), mode, rc, rh, rv, rrc)
    assert got.dtype == torch.int32 and got.device.type == "cpu" and got.shape == (16, 10)
    assert torch.equal(got, want)
    assert torch.equal(tf.check_geometry(got, 16, H, W), got)                     # a draw is always valid
    if mode == "short_side":
        assert len(set(got[:, 4].tolist())) > 4 and set(got[:, 4].tolist()) <= set(range(64, 97))
    if mode == "rrc":
        assert len(set(map(tuple, got[:, :4].tolist()))) == 16 and (got[:, 4:8] == torch.tensor([S, S, 0, 0])).all()
    # a switch that is off consumes nothing: the generator ends where the literal sequence ends
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    TF.TransformFrames(OPTS, generator=g1, **kw).draw_geometry(5, H, W)
    literal_geometry(ptx, 5, H, W, g2, mode, rc, rh, rv, rrc)
    assert torch.equal(g1.get_state(), g2.get_state())
    if mode == "plain" and not (rc or rh or rv):
        assert torch.equal(g1.get_state(), torch.Generator().manual_seed(3).get_state())
    # generator=None: torch's default CPU generator
    state = torch.get_rng_state()
    try:
        torch.manual_seed(77)
        a = TF.TransformFrames(OPTS, **kw).draw_geometry(6, H, W)
        torch.manual_seed(77)
        b = literal_geometry(ptx, 6, H, W, None, mode, rc, rh, rv, rrc)
    finally:
        torch.set_rng_state(state)
    assert torch.equal(a, b)


def test_random_resized_crop_exhausted_attempts_and_all_fallback_branches(ptx):
    TF = ptx.transforms
    # scale = (4, 4): every attempt asks for four times the frame's area and is rejected; the fallback draws nothing more
    for (Hh, Ww), box in (((90, 120), (0, 0, 90, 120)),          # in_ratio 4/3 inside the bounds: the whole frame
                          ((200, 100), (33, 0, 133, 100)),       # in_ratio 0.5 < 3/4: full width, h = round(100 / 0.75)
                          ((64, 2100), (0, 1007, 64, 85))):      # in_ratio > 4/3: full height, w = round(64 * 4/3)
        g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        tf = TF.TransformFrames(OPTS, random_resized_crop=dict(scale=(4, 4)), random_hflip=True, generator=g1)
        got = tf.draw_geometry(3, Hh, Ww)
        assert got[:, :8].tolist() == [list(box) + [S, S, 0, 0]] * 3, (Hh, Ww, got.tolist())
        for _ in range(3):
            assert literal_box(Hh, Ww, (4.0, 4.0), RATIO, g2) == box
            torch.rand(1, generator=g2)
        assert torch.equal(g1.get_state(), g2.get_state())                        # 10 x 2 uniforms + the flip per clip
    assert TF.random_resized_crop_box(90, 120, (4, 4), RATIO, torch.Generator().manual_seed(1)) == (0, 0, 90, 120)


def test_check_geometry_accepts_and_rejects(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    tf = TF.TransformFrames(OPTS, out="frames")
    ok = [[0, 0, 90, 120, 73, 97, 9, 33, 1, 1], [89, 119, 1, 1, 64, 64, 0, 0, 0, 0]]
    for form in (ok, np.array(ok), np.array(ok, np.int64), np.array(ok, np.uint8), torch.tensor(ok), torch.tensor(ok, dtype=torch.int32)):
        got = tf.check_geometry(form, 2, H, W)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and got.tolist() == ok
    good = ok[0]

    def bad(**kw):
        row = list(good)
        for k, v in kw.items():
            row[TF.GEOMETRY_FIELDS.index(k)] = v
        return [row]

    for g, n, match in (
            (np.zeros((1, 10), np.float32), 1, "must hold integers"),
            ([[0] * 9], 1, r"must be \[N, 10\]"),
            ([0] * 10, 1, r"must be \[N, 10\]"),
            (ok, 3, "geometry holds 2 clips, the frames hold N = 3"),
            (bad(box_h=0), 1, r"geometry\[0\]: the 0x120 box at \(0, 0\) is empty or does not lie inside the 90x120 frame"),
            (bad(box_w=0), 1, "is empty or does not lie inside"),
            (bad(box_top=-1), 1, "is empty or does not lie inside"),
            (bad(box_top=1), 1, "is empty or does not lie inside"),
            (bad(box_left=1), 1, "is empty or does not lie inside"),
            (bad(h=63, top=0), 1, r"geometry\[0\]: a 64x64 crop does not fit the resized 63x97 box"),
            (bad(w=63, left=0), 1, "a 64x64 crop does not fit the resized 73x63 box"),
            (bad(top=10), 1, r"geometry\[0\]: the 64x64 crop at \(10, 33\) does not fit the resized 73x97 box"),
            (bad(left=34), 1, "does not fit the resized 73x97 box"),
            (bad(top=-1), 1, "does not fit the resized 73x97 box"),
            (bad(hflip=2), 1, r"geometry\[0\]: a flip must be 0 or 1, got hflip=2 vflip=1"),
            (bad(vflip=-1), 1, "a flip must be 0 or 1"),
            ([ok[1], bad(box_h=1)[0]][::-1] + [ok[1]], 3, None)):                  # a one-row box is fine
        if match is None:
            tf.check_geometry(g, n, H, W)
            continue
        with pytest.raises(E, match=match):
            tf.check_geometry(g, n, H, W)
    # the tap cap: 2100 -> 64 needs 66 taps
    with pytest.raises(E, match=r"geometry\[1\]: down-scaling 2100 columns to 64 needs 66 taps, the kernel's cap is PTX_RESIZE_MAX_TAPS = 64"):
        tf.check_geometry([[0, 0, 64, 100, 64, 64, 0, 0, 0, 0], [0, 0, 64, 2100, 64, 64, 0, 0, 0, 0]], 2, 64, 2100)
    with pytest.raises(E, match=r"down-scaling 2100 rows to 64 needs 66 taps"):
        tf.check_geometry([[0, 0, 2100, 64, 64, 64, 0, 0, 0, 0]], 1, 2100, 64)
    assert TF.resize_axis_table(2100, 64)[2].shape[1] == 66


def test_the_host_tap_pitch_is_the_table_builders(ptx):
    """The product path sizes the device tables from lo / hi alone: that pitch must be the widest entry of the clip's window."""
    TF = ptx.transforms
    tf = TF.TransformFrames(OPTS, out="frames")
    rows = [[0, 0, 600, 200, 64, 64, 0, 0, 0, 0], [300, 100, 300, 100, 80, 108, 16, 44, 0, 1], [0, 0, 64, 200, 64, 64, 0, 0, 0, 0],
            [5, 7, 20, 17, 64, 64, 0, 0, 1, 1], [0, 0, 600, 200, 1830, 610, 1000, 300, 0, 0], [599, 199, 1, 1, 64, 64, 0, 0, 0, 0]]
    for row in rows:
        t = TF.geometry_tables(row, S)
        _, th, tw = tf._checked_geometry([row], 1, 600, 200)
        assert (th, tw) == (int(t["rows"][1].max()), int(t["cols"][1].max())) == (t["rows"][2].shape[1], t["cols"][2].shape[1]), row
    _, th, tw = tf._checked_geometry(rows, len(rows), 600, 200)
    assert (th, tw) == (19, 7)


def test_constructor_conflicts_and_call_conflicts(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    T = TF.TransformFrames
    for kw, match in (
            (dict(random_short_side=(63, 80)), "a >= 64"),
            (dict(random_short_side=(80, 70)), "pair of integers"),
            (dict(random_short_side=80), "pair of integers"),
            (dict(random_short_side=(64.0, 80)), "pair of integers"),
            (dict(random_short_side=(64, 80), preserve_aspect_ratio=False), "preserve_aspect_ratio=True"),
            (dict(random_short_side=(64, 80), crop=(0, 0)), "cannot be combined with crop"),
            (dict(random_resized_crop=True, random_crop=True), "cannot be combined with random_crop"),
            (dict(random_resized_crop=True, random_short_side=(64, 80)), "cannot be combined with random_short_side"),
            (dict(random_resized_crop=True, crop=(0, 0)), "cannot be combined with crop"),
            (dict(random_resized_crop=dict(size=3)), "takes scale and ratio"),
            (dict(random_resized_crop=dict(scale=(0.0, 1.0))), "scale must be a pair 0 < lo <= hi"),
            (dict(random_resized_crop=dict(ratio=(2.0, 1.0))), "ratio must be a pair 0 < lo <= hi"),
            (dict(random_resized_crop="yes"), "must be True or dict")):
        with pytest.raises(E, match=match):
            T(OPTS, **kw)
    # accepted forms; scale / preserve_aspect_ratio are ignored by random_resized_crop; flips combine with both
    assert T(OPTS, random_short_side=(64, 64)).random_short_side == (64, 64)
    assert T(OPTS, random_short_side=[70, 90], random_crop=True, hflip=True, random_vflip=True).per_clip_geometry
    r = T(OPTS, 0.5, False, random_resized_crop=dict(scale=(0.3, 1)), vflip=True, random_hflip=True)
    assert r.random_resized_crop == dict(scale=(0.3, 1.0), ratio=RATIO) and r.last_geometry is None
    plain = T(OPTS)
    assert not plain.per_clip_geometry and plain.random_short_side is None and plain.random_resized_crop is None
    assert not T(OPTS, random_resized_crop=False).per_clip_geometry
    # the positional order of the constructor is what it was
    p = T(OPTS, 0.8, True, (1, 2), True, "frames", torch.float32)
    assert (p.scale, p.crop, p.hflip, p.out) == (0.8, (1, 2), True, "frames")
    # the call: params= plus geometry=, params= on a per-clip-geometry transform; validation precedes the device
    cpu = torch.zeros(1, 1, H, W, 3, dtype=torch.uint8)
    g = plain.draw_geometry(1, H, W)
    assert g.tolist() == [[0, 0, 90, 120, 73, 97, 4, 16, 0, 0]]
    with pytest.raises(E, match="cannot be combined"):
        plain(cpu, params=[[0, 0, 0, 0]], geometry=g)
    with pytest.raises(E, match="pass geometry="):
        T(OPTS, random_short_side=(64, 80))(cpu, params=[[0, 0, 0, 0]])
    with pytest.raises(E, match="does not fit the resized 73x97 box"):
        plain(cpu, geometry=[[0, 0, 90, 120, 73, 97, 10, 16, 0, 0]])
    with pytest.raises(E, match="N = 1"):
        plain(cpu[0], geometry=g.repeat(2, 1))
    with pytest.raises(E, match="CUDA"):
        plain(cpu, geometry=g)                                                     # a valid geometry: only then the device
    with pytest.raises(E, match="CUDA"):
        T(OPTS, random_resized_crop=True)(cpu)
    assert plain.last_geometry is None and plain.last_params is None
    with pytest.raises(E, match="is empty or does not lie inside"):               # a YUV source is validated the same way
        plain(TF.YUV420(torch.zeros(1, 1, 90, 120, dtype=torch.uint8), torch.zeros(1, 1, 45, 60, 2, dtype=torch.uint8)),
              geometry=[[0, 0, 91, 120, 73, 97, 4, 16, 0, 0]])
    # params= / check_params / last_params are what they were
    with pytest.raises(E, match=r"params must be \[N, 4\] \(top, left, hflip, vflip\)"):
        plain.check_params([[0] * 10], 1, H, W)
    assert plain.check_params([[9, 33, 1, 1]], 1, H, W).tolist() == [[9, 33, 1, 1]]


@pytest.mark.parametrize("Hh,Ww,kw", [(90, 120, {}), (120, 90, dict(hflip=True)), (73, 97, dict(vflip=True)),
                                      (540, 960, dict(crop=(3, 40))), (100, 100, dict(scale=1.0, preserve_aspect_ratio=False))])
def test_the_default_equivalent_geometry_reproduces_build_tables(ptx, Hh, Ww, kw):
    """box = frame, (h, w) = resized_size(..), the constructor's window and flips: entry for entry build_tables' tables."""
    TF = ptx.transforms
    tf = TF.TransformFrames(OPTS, **kw)
    g = tf.draw_geometry(2, Hh, Ww)
    h, w = TF.resized_size(Hh, Ww, OPTS["input_size"], tf.scale, tf.preserve_aspect_ratio)
    top, left = TF.crop_window(h, w, S, tf.crop)
    assert g.tolist() == [[0, 0, Hh, Ww, h, w, top, left, int(tf.hflip), int(tf.vflip)]] * 2
    want, got = tf.tables(Hh, Ww), TF.geometry_tables(g[0].tolist(), S)
    for a, b in zip(want["rows"] + want["cols"], got["rows"] + got["cols"]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    assert got["resized"] == want["resized"] and got["window"] == want["window"]


def test_entry_points_check_on_the_host(ptx):
    """Null pointers, extents and the tap cap are refused before a device is needed."""
    L = ptx._lib
    lib = L.lib()
    d = L.ResizeDesc(2, 1, 90, 120, 3, 64, 64, 3, 3, L.PTX_RESIZE_OUT_U8)
    assert lib.ptx_resize_frames_u8_tables_supported(C.byref(d)) == 1
    one = C.c_void_p(16)
    assert lib.ptx_resize_build_tables(C.byref(d), None, one, one, one, one, one, one, None) == 1
    assert b"null pointer" in lib.ptx_last_error()
    assert lib.ptx_resize_build_tables(C.byref(d), one, one, one, None, one, one, one, None) == 1
    assert lib.ptx_resize_frames_u8_tables(C.byref(d), one, one, one, one, one, one, None, one, None, None) == 1
    assert b"ptx_resize_frames_u8_tables: null pointer" in lib.ptx_last_error()
    assert lib.ptx_resize_frames_yuv420_tables(C.byref(d), None, one, one, one, one, one, one, one, None, None) == 1
    assert b"null source descriptor" in lib.ptx_last_error()
    big = L.ResizeDesc(2, 1, 90, 120, 3, 64, 64, 3, L.PTX_RESIZE_MAX_TAPS + 1, L.PTX_RESIZE_OUT_U8)
    assert lib.ptx_resize_frames_u8_tables_supported(C.byref(big)) == 0
    assert lib.ptx_resize_build_tables(C.byref(big), one, one, one, one, one, one, one, None) == 2
    assert b"PTX_RESIZE_MAX_TAPS" in lib.ptx_last_error()
    src = L.Yuv420Src()
    assert lib.ptx_resize_frames_yuv420_tables_supported(C.byref(d), C.byref(src)) == 0      # null planes
    assert C.sizeof(L.ResizeGeom) == 40 and [n for n, _ in L.ResizeGeom._fields_] == list(ptx.transforms.GEOMETRY_FIELDS)
