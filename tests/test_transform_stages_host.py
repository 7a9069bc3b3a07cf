"""Host test (no GPU) of the stage runner behind the resize of TransformFrames / SampleClips (`pretorched.transforms._apply_stages`):
for every non-empty subset of colour, blur, augment and mix and every output, the stages run and draw in the order colour, blur,
augment, mix; every stage but the last writes uint8 frames without a norm and the last one the call's output; the result has the
rank of the input; a replay with given params draws nothing.  The stages are the real classes with the launch alone replaced by
a recorder, so the draws and the params checks are the product's host code."""
import itertools

import pytest
import torch

OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 8, 8])
ORDER = ("color", "blur", "augment", "mix")
SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(ORDER, r)]
OUTS = [("tensor", torch.float32), ("tensor", torch.bfloat16), ("frames", torch.float32)]
SHAPES = [(2, 2, 8, 8, 3), (2, 8, 8, 3), (8, 8, 3)]
SEED = 1234


def make_stages(TF, generator, log=None):
    """The four stages on one generator.  With `log`, their launches are recorders of (name, mode, norm is None, dtype) that
    return a CPU tensor of the launch's shape and dtype."""
    U8 = TF._lib.PTX_RESIZE_OUT_U8

    def result(f5, mode, dtype):
        N, T, H, W, _ = f5.shape
        return torch.zeros((N, T, H, W, 3), dtype=torch.uint8) if mode == U8 else torch.zeros((N, 3, T, H, W), dtype=dtype)

    def recorder(cls, name):
        if log is None:
            return cls

        class Recorder(cls):
            def _launch(self, f5, params, mode, norm, dtype):
                log.append((name, mode, norm is None, dtype))
                return result(f5, mode, dtype)
        return Recorder

    class MixRecorder(TF.BatchMix):
        def _launch(self, src, src_mode, out_mode, N, T, H, W, dtype, norm, rows, noise_elems, noise=None):
            assert src_mode == TF._lib.PTX_MIX_SRC_U8
            log.append(("mix", out_mode, norm is None, dtype))
            return result(src, out_mode, dtype)

    return {"color": recorder(TF.ColorJitter, "color")(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=generator),
            "blur": recorder(TF.GaussianBlur, "blur")(3, p=0.5, generator=generator),
            "augment": recorder(TF.RandAugment, "augment")(generator=generator),
            "mix": (TF.BatchMix if log is None else MixRecorder)(mode="clip", generator=generator)}


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def test_the_order_is_stated_once(ptx):
    assert ptx.transforms._STAGES == ORDER and len(SUBSETS) == 15


@pytest.mark.parametrize("subset", SUBSETS, ids="+".join)
def test_stage_runner(ptx, subset):
    TF = ptx.transforms
    U8, F32, BF16 = TF._lib.PTX_RESIZE_OUT_U8, TF._lib.PTX_RESIZE_OUT_F32, TF._lib.PTX_RESIZE_OUT_BF16
    norm = TF.FramesToTensor(OPTS).norm
    for (out, dtype), shape in itertools.product(OUTS, SHAPES):
        if "mix" in subset and out == "frames":                     # 8 of the 15 subsets: refused where the stages are given
            kw = {name: stage for name, stage in make_stages(TF, None).items() if name in subset}
            for cls in (TF.TransformFrames, TF.SampleClips):
                with pytest.raises(ptx._lib.PtxError, match="%s: mix= needs out='tensor'" % cls.__name__):
                    cls(OPTS, out="frames", **kw)
            continue
        g, log = torch.Generator().manual_seed(SEED), []
        stages = {name: stage for name, stage in make_stages(TF, g, log).items() if name in subset}
        frames = torch.zeros(shape, dtype=torch.uint8)
        y = TF._apply_stages(stages, frames, out, dtype, norm, {})

        last_mode = U8 if out == "frames" else (F32 if dtype == torch.float32 else BF16)
        want = [(name, U8, True, torch.uint8) for name in subset[:-1]]
        want.append((subset[-1], last_mode, out == "frames", torch.uint8 if out == "frames" else dtype))
        assert log == want, (subset, out, dtype, shape)

        N, T = (shape[0] if len(shape) == 5 else 1), (shape[-4] if len(shape) >= 4 else 1)
        if out == "frames":
            assert y.dtype == torch.uint8 and tuple(y.shape) == shape
        else:
            assert y.dtype == dtype and tuple(y.shape) == ((N, 3, T, 8, 8), (3, T, 8, 8), (3, 8, 8))[5 - len(shape)]

        g2 = torch.Generator().manual_seed(SEED)                     # the draw order: the public draws, in the stages' order
        ref = make_stages(TF, g2)
        for name in subset:
            drawn = ref[name].draw(N) if name in ("color", "blur") else ref[name].draw(N, 8, 8)
            assert same(stages[name].last_params, drawn), (subset, name)
        assert torch.equal(g.get_state(), g2.get_state())

        state, drawn = g.get_state(), {name: stages[name].last_params for name in subset}
        del log[:]
        y2 = TF._apply_stages(stages, frames, out, dtype, norm, dict(drawn))
        assert log == want and y2.shape == y.shape and torch.equal(g.get_state(), state)
        assert all(stages[name].last_params is drawn[name] for name in subset)
