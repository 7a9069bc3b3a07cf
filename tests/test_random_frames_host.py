"""No-GPU tests of per-clip crop windows and flips in `pretorched.transforms.TransformFrames` (`random_crop`, `random_hflip`,
`random_vflip`, `vflip`, `params=`): the draw against the literal torch call sequence, the validation of given parameters
and of the constructor, the tables (a flip is a reversed slice of the whole-frame tables), the stored cases
(tests/golden/random_frames.npz, written by tests/golden/make_random_frames_golden.py with PIL only) against the numpy model,
and the host-side checks of the C entry points."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_frames

OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])
S, H, W, RH, RW = 64, 90, 120, 73, 97                                   # 90 x 120 frames resize to 73 x 97


def literal_draw(N, h, w, g, rc, rh, rv, fixed):
    """The contract, call by call: per clip randint (top), randint (left), rand (hflip), rand (vflip) for the switches on."""
    out = []
    for _ in range(N):
        top, left, hf, vf = fixed
        if rc:
            top = int(torch.randint(0, h - S + 1, (1,), generator=g))
            left = int(torch.randint(0, w - S + 1, (1,), generator=g))
        if rh:
            hf = int(torch.rand(1, generator=g) < 0.5)
        if rv:
            vf = int(torch.rand(1, generator=g) < 0.5)
        out.append([top, left, hf, vf])
    return torch.tensor(out, dtype=torch.int32)


@pytest.mark.parametrize("rc,rh,rv", list(itertools.product((False, True), repeat=3)))
def test_draw_is_the_literal_torch_sequence(ptx, rc, rh, rv):
    TF = ptx.transforms
    kw = dict(random_crop=rc, random_hflip=rh, random_vflip=rv)
    tf = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(11), **kw)
    got = tf.draw(16, H, W)
    want = literal_draw(16, RH, RW, torch.Generator().manual_seed(11), rc, rh, rv, (4, 16, 0, 0))   # centre of 73 x 97
    assert got.dtype == torch.int32 and got.device.type == "cpu" and got.shape == (16, 4)
    assert torch.equal(got, want)
    # the same seed repeats, a second draw continues the stream
    again = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(11), **kw)
    assert torch.equal(again.draw(16, H, W), got)
    if rc or rh or rv:
        assert not torch.equal(tf.draw(16, H, W), got)
    # ranges
    assert int(got[:, 0].min()) >= 0 and int(got[:, 0].max()) <= RH - S and int(got[:, 1].min()) >= 0 and int(got[:, 1].max()) <= RW - S
    assert set(got[:, 2:].reshape(-1).tolist()) <= {0, 1}
    if rc:
        assert len(set(got[:, 1].tolist())) > 4                                   # 34 possible columns: the draws differ
    # switches that are off consume nothing: the generator ends where the literal sequence ends
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    TF.TransformFrames(OPTS, generator=g1, **kw).draw(5, H, W)
    literal_draw(5, RH, RW, g2, rc, rh, rv, (4, 16, 0, 0))
    assert torch.equal(g1.get_state(), g2.get_state())
    if not (rc or rh or rv):
        assert torch.equal(g1.get_state(), torch.Generator().manual_seed(3).get_state())
    # generator=None: torch's default CPU generator, torch.manual_seed governs
    state = torch.get_rng_state()
    try:
        torch.manual_seed(77)
        a = TF.TransformFrames(OPTS, **kw).draw(6, H, W)
        torch.manual_seed(77)
        b = literal_draw(6, RH, RW, None, rc, rh, rv, (4, 16, 0, 0))
    finally:
        torch.set_rng_state(state)
    assert torch.equal(a, b)


def test_draw_uses_the_constructor_values_for_switches_that_are_off(ptx):
    TF = ptx.transforms
    g = torch.Generator().manual_seed(1)
    tf = TF.TransformFrames(OPTS, crop=(9, 33), hflip=True, random_vflip=True, generator=g)
    p = tf.draw(8, H, W)
    assert p[:, :3].tolist() == [[9, 33, 1]] * 8 and set(p[:, 3].tolist()) == {0, 1}
    tf = TF.TransformFrames(OPTS, vflip=True, random_crop=True, random_hflip=True, generator=g)
    p = tf.draw(8, H, W)
    assert p[:, 3].tolist() == [1] * 8 and len(set(map(tuple, p[:, :2].tolist()))) > 1
    # portrait frames: the roles of the axes swap; a frame that holds exactly one window always draws (0, 0)
    p = TF.TransformFrames(OPTS, random_crop=True, generator=g).draw(8, 120, 90)
    assert int(p[:, 0].max()) <= 97 - S and int(p[:, 1].max()) <= 73 - S
    p = TF.TransformFrames(OPTS, scale=1.0, random_crop=True, generator=g).draw(4, 64, 64)
    assert p.tolist() == [[0, 0, 0, 0]] * 4
    with pytest.raises(ptx._lib.PtxError, match="does not fit"):
        TF.TransformFrames(OPTS, scale=2.0, random_crop=True).draw(1, H, W)        # resized to 32 x 42: no 64 x 64 window


def test_constructor_and_params_validation(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    with pytest.raises(E, match="random_crop"):
        TF.TransformFrames(OPTS, crop=(0, 0), random_crop=True)
    with pytest.raises(E, match="random_hflip"):
        TF.TransformFrames(OPTS, hflip=True, random_hflip=True)
    with pytest.raises(E, match="random_vflip"):
        TF.TransformFrames(OPTS, vflip=True, random_vflip=True)
    with pytest.raises(E, match="generator"):
        TF.TransformFrames(OPTS, random_crop=True, generator=5)
    with pytest.raises(TypeError):
        TF.TransformFrames(OPTS, 0.875, True, "center", False, "tensor", torch.float32, True)   # the new switches are keyword-only
    tf = TF.TransformFrames(OPTS, 0.875, True, "center", True, "frames", torch.float32)         # the positional order holds
    assert (tf.hflip, tf.vflip, tf.out, tf.random, tf.last_params) == (True, False, "frames", False, None)
    assert TF.TransformFrames(OPTS, random_crop=True, hflip=True, vflip=True).random
    # params: accepted forms come back as a CPU int32 tensor
    good = [[0, 0, 0, 0], [9, 33, 1, 1]]
    for p in (np.array(good), np.array(good, np.int32), torch.tensor(good), torch.tensor(good, dtype=torch.int32), good):
        got = tf.check_params(p, 2, H, W)
        assert got.dtype == torch.int32 and got.tolist() == good
    for bad, msg in (([[10, 0, 0, 0], [0, 0, 0, 0]], "does not fit"), ([[0, 0, 0, 0], [0, 34, 0, 0]], "does not fit"),
                     ([[-1, 0, 0, 0], [0, 0, 0, 0]], "does not fit"), ([[0, -1, 0, 0], [0, 0, 0, 0]], "does not fit"),
                     ([[0, 0, 2, 0], [0, 0, 0, 0]], "flip"), ([[0, 0, 0, 0], [0, 0, 0, -1]], "flip"),
                     ([[0, 0, 0, 0]], "N = 2"), ([[0, 0, 0, 0]] * 3, "N = 2"), ([[0, 0, 0], [0, 0, 0]], r"\[N, 4\]"),
                     ([0, 0, 0, 0], r"\[N, 4\]"), (np.zeros((2, 4), np.float32), "integers"), (np.zeros((2, 4), bool), "integers")):
        with pytest.raises(E, match=msg):
            tf.check_params(bad, 2, H, W)
    with pytest.raises(E, match="does not fit"):
        tf.check_params([[0, 33, 0, 0]], 1, 120, 90)                                # fits 73 x 97, not the portrait 97 x 73
    assert tf.check_params([[33, 0, 0, 0]], 1, 120, 90).tolist() == [[33, 0, 0, 0]]
    # the call validates before it touches a device
    with pytest.raises(E, match="CUDA"):
        TF.TransformFrames(OPTS, random_crop=True)(torch.zeros(1, 1, H, W, 3, dtype=torch.uint8))
    # what stays refused
    with pytest.raises(E):
        TF.SampleViews(OPTS, sampling="random")
    with pytest.raises(E):
        TF.SampleViews(OPTS, crops=5)


def test_tables_vflip_and_whole_frame(ptx):
    TF = ptx.transforms
    plain = TF.build_tables(H, W, [3, 64, 64], crop=(4, 17))
    flipped = TF.build_tables(H, W, [3, 64, 64], 0.875, True, (4, 17), False, True)          # trailing positional vflip
    for a, b in zip(plain["rows"], flipped["rows"]):
        assert np.array_equal(a[::-1], b)
    for a, b in zip(plain["cols"], flipped["cols"]):
        assert np.array_equal(a, b)
    assert flipped["window"] == (4, 17) and flipped["resized"] == (RH, RW)
    tf = TF.TransformFrames(OPTS, crop=(4, 17), vflip=True, hflip=True)
    both = tf.tables(H, W)
    for a, b in zip(plain["rows"] + plain["cols"], both["rows"] + both["cols"]):
        assert np.array_equal(a[::-1], b)
    # the whole-frame tables: every window of build_tables is a slice of them
    full = tf.frame_tables(H, W)
    assert full["resized"] == (RH, RW) and full["S"] == S
    assert [len(a) for a in full["rows"]] == [RH] * 3 and [len(a) for a in full["cols"]] == [RW] * 3
    for (top, left, hf, vf) in ((0, 0, 0, 0), (9, 33, 1, 0), (4, 17, 0, 1), (9, 0, 1, 1)):
        t = TF.build_tables(H, W, [3, 64, 64], crop=(top, left), hflip=bool(hf), vflip=bool(vf))
        rows = tuple(a[top:top + S][::-1] if vf else a[top:top + S] for a in full["rows"])
        cols = tuple(a[left:left + S][::-1] if hf else a[left:left + S] for a in full["cols"])
        for a, b in zip(rows + cols, t["rows"] + t["cols"]):
            assert np.array_equal(a[..., :b.shape[-1]] if a.ndim == 2 else a, b)
    with pytest.raises(ptx._lib.PtxError, match="does not fit"):
        TF.build_frame_tables(H, W, [3, 64, 64], scale=2.0)
    with pytest.raises(ptx._lib.PtxError, match="PTX_RESIZE_MAX_TAPS"):
        TF.build_frame_tables(40 * 74, 40 * 74, [3, 64, 64])


def test_numpy_model_on_per_clip_slices_equals_stored_cases(ptx):
    TF = ptx.transforms
    blob = load_golden("random_frames")
    cases = json.loads(str(blob["cases"]))
    assert [c["name"] for c in cases] == ["landscape_90x120", "portrait_120x90", "crop_only_73x97", "down_540x960", "wide_64x2100"]
    want_params = {"landscape_90x120": [[0, 0, 0, 0], [9, 33, 1, 0], [4, 17, 0, 1], [9, 0, 1, 1]],
                   "portrait_120x90": [[33, 9, 1, 1], [0, 5, 0, 0], [16, 0, 0, 1]],
                   "crop_only_73x97": [[9, 33, 1, 1], [0, 1, 0, 0]],
                   "down_540x960": [[0, 65, 0, 1], [9, 0, 1, 0]],
                   "wide_64x2100": [[0, 2331, 1, 0], [9, 1100, 0, 1]]}
    want_shape = {"landscape_90x120": ([73, 97], [3, 3], 2), "portrait_120x90": ([97, 73], [3, 3], 1),
                  "crop_only_73x97": ([73, 97], [1, 1], 1), "down_540x960": ([73, 129], [15, 15], 1),
                  "wide_64x2100": ([73, 2395], [2, 2], 1)}
    for c in cases:
        assert c["params"] == want_params[c["name"]] and (c["resized"], c["taps"], c["T"]) == want_shape[c["name"]]
        assert c["input_size"] == [3, 64, 64]
        N, T = len(c["params"]), c["T"]
        frames = synth_frames(N * T, c["H"], c["W"], c["seed"]).reshape(N, T, c["H"], c["W"], 3)
        full = TF.build_frame_tables(c["H"], c["W"], c["input_size"])
        assert list(full["resized"]) == c["resized"]
        assert [full["rows"][2].shape[1], full["cols"][2].shape[1]] == c["taps"]
        want = blob["out_" + c["name"]]
        assert want.shape == (N, T, S, S, 3) and want.dtype == np.uint8
        tf = TF.TransformFrames(OPTS)
        assert tf.check_params(c["params"], N, c["H"], c["W"]).tolist() == c["params"]
        for n, (top, left, hf, vf) in enumerate(c["params"]):
            tables = {"rows": tuple(np.ascontiguousarray(a[top:top + S][::-1] if vf else a[top:top + S]) for a in full["rows"]),
                      "cols": tuple(np.ascontiguousarray(a[left:left + S][::-1] if hf else a[left:left + S]) for a in full["cols"])}
            for t in range(T):
                assert np.array_equal(TF.apply_tables_numpy(frames[n, t], tables), want[n, t]), (c["name"], n, t)
    # the windows of the first case differ from each other: a launch that ignored the parameters cannot pass
    first = blob["out_landscape_90x120"]
    assert all(not np.array_equal(first[0], first[n]) for n in (1, 2, 3))


def test_windows_abi_host_checks(ptx):
    L = ptx._lib
    lib = L.lib()
    names = ("ptx_resize_frames_u8_windows", "ptx_resize_frames_u8_windows_supported", "ptx_resize_frames_yuv420_windows",
             "ptx_resize_frames_yuv420_windows_supported")
    for name in names:
        assert name in L.header_symbols() and name in L.SIGNATURES and name not in L.EXPERIMENTAL
        assert name not in L.experimental_symbols() and hasattr(lib, name)
    assert [n for n, _ in L.ResizeWindow._fields_] == ["top", "left", "hflip", "vflip"] and C.sizeof(L.ResizeWindow) == 16
    text = open(L.HEADER_PATH).read()
    assert "typedef struct ptx_resize_window {" in text
    assert C.sizeof(L.ResizeDesc) == 40                                             # the descriptor's layout did not change

    P = 64                                                  # never dereferenced: every call below returns before a launch
    good = (2, 4, 90, 120, 3, 64, 64, 3, 3, L.PTX_RESIZE_OUT_U8)

    def err(who="windows"):
        msg = lib.ptx_last_error().decode()
        assert who in msg
        return msg

    def src(**kw):
        s = L.Yuv420Src()
        s.y, s.u, s.v = P, 2 * P, 2 * P + 1
        s.stride_n_y, s.stride_t_y, s.stride_n_c, s.stride_t_c = 4 * 90 * 120, 90 * 120, 4 * 45 * 120, 45 * 120
        s.pitch_y, s.pitch_c, s.step_c = 120, 120, 2
        s.y_off, s.ky, s.krv, s.kgu, s.kgv, s.kbu = 16, 76309, 117489, 13975, 34925, 138438
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    ok = lib.ptx_resize_frames_u8_windows_supported
    assert ok(C.byref(L.ResizeDesc(*good)), 73, 97) == 1
    assert ok(C.byref(L.ResizeDesc(*good)), 64, 64) == 1                            # exactly one window
    assert ok(C.byref(L.ResizeDesc(*good)), 63, 97) == 0 and "does not fit" in err()
    assert ok(C.byref(L.ResizeDesc(*good)), 73, 63) == 0 and "does not fit" in err()
    assert ok(None, 73, 97) == 0 and "null" in err()
    d = L.ResizeDesc(*good)
    d.taps_w = L.PTX_RESIZE_MAX_TAPS + 1
    assert ok(C.byref(d), 73, 97) == 0 and "PTX_RESIZE_MAX_TAPS" in err()          # everything resize_plan checks
    assert ok(C.byref(L.ResizeDesc(*good)), 1 << 30, 97) == 0 and "32-bit" in err()
    yok = lib.ptx_resize_frames_yuv420_windows_supported
    assert yok(C.byref(L.ResizeDesc(*good)), C.byref(src()), 73, 97) == 1
    assert yok(C.byref(L.ResizeDesc(*good)), C.byref(src()), 73, 10) == 0 and "does not fit" in err()
    assert yok(C.byref(L.ResizeDesc(*good)), None, 73, 97) == 0 and "null" in err()
    assert yok(C.byref(L.ResizeDesc(*good)), C.byref(src(pitch_y=119)), 73, 97) == 0 and "shorter than a row" in err()

    # the launching calls run the same checks first and return a status
    tables = (C.c_void_p(P),) * 6

    def call(d, frames=C.c_void_p(P), h=73, w=97, wins=C.c_void_p(P), y=C.c_void_p(P), tab=tables):
        return lib.ptx_resize_frames_u8_windows(C.byref(d), frames, *tab, h, w, wins, y, None, None)

    def ycall(d, s, h=73, w=97, wins=C.c_void_p(P), y=C.c_void_p(P)):
        return lib.ptx_resize_frames_yuv420_windows(C.byref(d), C.byref(s) if s is not None else None, *tables, h, w, wins, y, None, None)

    assert call(L.ResizeDesc(*good), h=63) == 1 and "does not fit" in err()
    assert call(L.ResizeDesc(*good), w=63) == 1 and "does not fit" in err()
    assert call(L.ResizeDesc(*good), wins=None) == 1 and "null pointer" in err()
    assert call(L.ResizeDesc(*good), frames=None) == 1 and "null pointer" in err()
    assert call(L.ResizeDesc(*good), y=None) == 1 and "null pointer" in err()
    for i in range(6):
        tab = tuple(None if j == i else C.c_void_p(P) for j in range(6))
        assert call(L.ResizeDesc(*good), tab=tab) == 1 and "null pointer" in err()
    d = L.ResizeDesc(*good)
    d.out_mode = L.PTX_RESIZE_OUT_F32
    assert call(d) == 1 and "norm" in err()
    d = L.ResizeDesc(*good)
    d.C = 5
    assert call(d) == 1 and "C=5" in err()
    assert ycall(L.ResizeDesc(*good), None) == 1 and "null" in err()
    assert ycall(L.ResizeDesc(*good), src(), h=10) == 1 and "does not fit" in err()
    assert ycall(L.ResizeDesc(*good), src(), wins=None) == 1 and "null pointer" in err()
    assert ycall(L.ResizeDesc(*good), src(step_c=3)) == 1 and "step_c" in err()
