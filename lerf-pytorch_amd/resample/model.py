"""The trainable models of the reference, on the MI355X path: mirror of `SWF2LUT` in resample/model.py:130-431
(`InterpTorchBatch`, `forward`, `predict`) -- LUT fine-tuning, scripts.sh:28-30 -- and of the hyper-networks
`SRNetsSWF2` (:69-129) that train_model.py --twoStage trains and transfer_to_lut turns into LUTs (`SRNetsSWF2`,
`export_srnets`; the nets run in lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32).

The LUT pass runs in liblerf_hip.so (lerf_swf2lut_interp_f32 / _bwd_f32) behind a torch.autograd.Function whose
backward is the gradient autograd derives for the reference code: into the LUT parameters (straight-through round,
clamp gate) and into the input through the LSB terms.  Everything else in `predict` (rot90, replicate pad, the
straight-through rounding between passes) is the reference's own torch glue.

Like the reference, modes "c" and "t" of this twin read their LSBs at the 'y' pattern pixels (model.py:229-232,
240-243); the deploy-time numpy pass (eval_lut_sr.FourSimplexInterpFaster) does not.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

mode_pad_dict = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3, "e": 3, "l": 3, "f": 4, "m": 4, "g": 5, "n": 5}


def round_func(input):
    """Backward-pass differentiable approximation of round (model.py:16-22)."""
    forward_value = torch.round(input)
    out = input.clone()
    out.data = forward_value.data
    return out


def _mode_char(mode):
    if not isinstance(mode, str) or len(mode) != 1 or mode not in "sdyct":
        raise ValueError("Mode {} not implemented.".format(mode))          # model.py:246
    return mode.encode()


class _InterpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, img_in, outC, mode, bd):
        if not (weight.is_cuda and img_in.is_cuda):
            raise ValueError("SWF2LUT runs on the GPU (there is no CPU path)")
        w = weight.detach().contiguous().float()
        x = img_in.detach().contiguous().float()
        B, Cn, hp, wp = x.shape
        h, wd = hp - bd, wp - bd
        if w.shape != (_lib.LERF_LUT_ENTRIES, outC):
            raise ValueError("weight must be [17^4, outC]")
        out = torch.empty((B, Cn * outC, h, wd), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().lerf_swf2lut_interp_f32(C.c_void_p(w.data_ptr()), int(outC), _mode_char(mode),
                                                      C.c_void_p(x.data_ptr()), B * Cn, h, wd, int(bd),
                                                      C.c_void_p(out.data_ptr()), _lib.current_stream()),
                   "lerf_swf2lut_interp_f32")
        ctx.save_for_backward(w, x)
        ctx.meta = (int(outC), mode, int(bd))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w, x = ctx.saved_tensors
        outC, mode, bd = ctx.meta
        B, Cn, hp, wp = x.shape
        g = grad_out.contiguous().float()
        gw = torch.zeros_like(w) if ctx.needs_input_grad[0] else None
        gx = torch.zeros_like(x) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().lerf_swf2lut_interp_bwd_f32(
            C.c_void_p(w.data_ptr()), outC, _mode_char(mode), C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr()),
            B * Cn, hp - bd, wp - bd, bd, C.c_void_p(gw.data_ptr() if gw is not None else None),
            C.c_void_p(gx.data_ptr() if gx is not None else None), _lib.current_stream()), "lerf_swf2lut_interp_bwd_f32")
        return gw, gx, None, None, None


class SWF2LUT(nn.Module):
    """model.py:130-431.  `opt` carries modes, modes2, stages, norm, interval, expDir (common/option.py:21-35);
    the LUT files are `<expDir>/<lutName>_s{stage}_{mode}r{r}.npy` with lutName = "LUT" like the reference
    (`opt.lutName` selects another prefix, e.g. the shipped "LUTft")."""

    def __init__(self, opt, inC=1, outC=3):
        super(SWF2LUT, self).__init__()
        self.modes2 = opt.modes2
        self.modes = opt.modes
        self.stages = opt.stages
        self.norm = opt.norm
        self.interval = opt.interval
        if self.interval != 4 or self.stages != 2:
            raise NotImplementedError("only interval=4, stages=2 (the shipped models) are implemented")
        name = getattr(opt, "lutName", None) or "LUT"
        self.outC = outC
        for mode in self.modes2:                                # hyper stage (:140-149)
            for r in [0, 1]:
                key = "s{}_{}r{}".format(2, mode, r)
                arr = np.load(os.path.join(opt.expDir, "{}_{}.npy".format(name, key))).reshape(-1, outC).astype(np.float32) / 127.0
                self.register_parameter(name="weight_" + key, param=torch.nn.Parameter(torch.Tensor(arr)))
        for mode in self.modes:                                 # stage 1 (:151-158)
            key = "s{}_{}r{}".format(1, mode, 0)
            arr = np.load(os.path.join(opt.expDir, "{}_{}.npy".format(name, key))).reshape(-1, 1).astype(np.float32) / 127.0
            self.register_parameter(name="weight_" + key, param=torch.nn.Parameter(torch.Tensor(arr)))

    round_func = staticmethod(round_func)

    def InterpTorchBatch(self, weight, outC, mode, img_in, bd):
        """[B, C, h+bd, w+bd] (integer-valued float32) -> [B, C*outC, h, w] (:172-385)."""
        _mode_char(mode)
        return _InterpFn.apply(weight, img_in, outC, mode, bd)

    def forward(self, x, stage, mode, r):
        key = "s{}_{}r{}".format(str(stage), mode, r)
        pad = mode_pad_dict[mode]
        outC = 1 if stage == 1 else self.outC
        return self.InterpTorchBatch(getattr(self, "weight_" + key), outC, mode, x, pad)

    def _rotation_ensemble(self, x, modes, stage, lut_of_rotation, scale=None):
        """Sum over modes and the four quarter-turns of one stage: rotate, replicate-pad bottom/right by the mode's
        reach, LUT pass, rotate back, straight-through round (model.py:405-412, 419-424).  `scale` multiplies the
        rotated-back pass before the round (SRNetsSWF2: the net's tanh output times norm//2, model.py:101-124)."""
        total = 0
        for mode in modes:
            reach = mode_pad_dict[mode]
            for quarter_turns in range(4):
                rotated = F.pad(torch.rot90(x, quarter_turns, [2, 3]), (0, reach, 0, reach), mode="replicate")
                passed = self.forward(rotated, stage=stage, mode=mode, r=lut_of_rotation(quarter_turns))
                back = torch.rot90(passed, (4 - quarter_turns) % 4, [2, 3])
                total = total + round_func(back if scale is None else back * scale)
        return total

    def predict(self, x, stage=None):
        """x in [0, 1]; stage 2 -> hyper-parameter maps in [0, 1] ([B, outC, H, W] per input channel), otherwise the
        pre-filtered image in 0..255 (model.py:398-431)."""
        x = round_func(x * 255.0)                                             # 8-bit input
        if stage == 2:
            # hyper stage: LUT r0 serves rotations 0 and 2, LUT r1 rotations 1 and 3; mean over 4 x modes, + 127
            pred = self._rotation_ensemble(x, self.modes2, self.stages, lambda q: q & 1)
            return torch.clamp(round_func(pred / (len(self.modes2) * 4) + self.norm // 2), 0, self.norm) / float(self.norm)
        # feature stage(s): one LUT per mode for all four rotations
        for s in range(self.stages - 1):
            pred = self._rotation_ensemble(x, self.modes, s + 1, lambda q: 0)
            if s + 1 == self.stages - 1:        # the last feature stage keeps the 0..255 range (divide by the modes only)
                x = torch.clamp(round_func(pred / len(self.modes)), 0, self.norm)
            else:
                x = torch.clamp(round_func(pred / (len(self.modes) * 4)) + self.norm // 2, 0, self.norm) / float(self.norm)
        return x


class _SRNetFn(torch.autograd.Function):
    """One SRNet on [B, C, h+bd, w+bd] planes -> tanh output [B, C*outC, h, w] (lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32);
    the weights arrive packed (torch.cat of the parameters, so autograd hands each parameter its slice of the packed
    gradient)."""

    @staticmethod
    def forward(ctx, flat, img_in, outC, mode, bd):
        if not (flat.is_cuda and img_in.is_cuda):
            raise ValueError("SRNetsSWF2 runs on the GPU (there is no CPU path)")
        w = flat.detach().contiguous().float()
        x = img_in.detach().contiguous().float()
        B, Cn, hp, wp = x.shape
        h, wd = hp - bd, wp - bd
        out = torch.empty((B, Cn * outC, h, wd), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().lerf_srnet_fwd_f32(C.c_void_p(w.data_ptr()), int(outC), _mode_char(mode), C.c_void_p(x.data_ptr()),
                                                 B * Cn, h, wd, int(bd), C.c_void_p(out.data_ptr()), _lib.current_stream()),
                   "lerf_srnet_fwd_f32")
        ctx.save_for_backward(w, x)
        ctx.meta = (int(outC), mode, int(bd))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w, x = ctx.saved_tensors
        outC, mode, bd = ctx.meta
        B, Cn, hp, wp = x.shape
        h, wd = hp - bd, wp - bd
        g = grad_out.contiguous().float()
        gw = torch.zeros_like(w)
        gx = torch.zeros_like(x) if ctx.needs_input_grad[1] else None
        L = _lib.lib()
        nbytes = L.lerf_srnet_bwd_workspace_bytes(outC, B * Cn, h, wd)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        _lib.check(L.lerf_srnet_bwd_f32(C.c_void_p(w.data_ptr()), outC, _mode_char(mode), C.c_void_p(x.data_ptr()),
                                        C.c_void_p(g.data_ptr()), B * Cn, h, wd, bd, C.c_void_p(gw.data_ptr()),
                                        C.c_void_p(gx.data_ptr() if gx is not None else None), C.c_void_p(ws.data_ptr()),
                                        nbytes, _lib.current_stream()), "lerf_srnet_bwd_f32")
        return (gw if ctx.needs_input_grad[0] else None), gx, None, None, None


class _Conv(nn.Module):
    """common/network.py:14-28: Conv2d with MSRA (Kaiming-normal) weights and zero biases; only its parameters are used
    here (the layer runs inside lerf_srnet_fwd_f32)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super(_Conv, self).__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size)
        nn.init.kaiming_normal_(self.conv.weight)
        nn.init.constant_(self.conv.bias, 0)


class _DenseConv(nn.Module):
    def __init__(self, in_nf, nf=64):                            # network.py:31-41
        super(_DenseConv, self).__init__()
        self.conv1 = _Conv(in_nf, nf, 1)


class _SRUnit(nn.Module):
    def __init__(self, mode, nf, outC):                          # network.py:43-71 (upscale 1)
        super(_SRUnit, self).__init__()
        self.conv1 = _Conv(1, nf, 2 if mode in "sd" else (1, 4))
        self.conv2 = _DenseConv(nf, nf)
        self.conv3 = _DenseConv(nf + nf * 1, nf)
        self.conv4 = _DenseConv(nf + nf * 2, nf)
        self.conv5 = _DenseConv(nf + nf * 3, nf)
        self.conv6 = _Conv(nf * 5, outC, 1)


class _SRNet(nn.Module):
    """network.py:74-163 for the modes sdyct at upscale 1: parameters under `model.`, the pass in HIP."""

    def __init__(self, mode, nf, outC):
        super(_SRNet, self).__init__()
        _mode_char(mode)
        self.mode = mode
        self.outC = outC
        self.model = _SRUnit(mode, nf, outC)

    def packed(self):
        """the parameters flattened in module order: the packed layout of lerf_srnet_fwd_f32"""
        return torch.cat([p.reshape(-1) for p in self.parameters()])

    def forward(self, x):
        return _SRNetFn.apply(self.packed(), x, self.outC, self.mode, mode_pad_dict[self.mode])


class SRNetsSWF2(nn.Module):
    """The trainable hyper-networks of the reference, resample/model.py:69-129 (train_model.py --twoStage, scripts.sh
    step 1): one SRNet per stage-1 mode (`s1_<mode>r0`, one output channel) and two per stage-2 mode (`s2_<mode>r0` for
    rotations 0 and 2, `s2_<mode>r1` for 1 and 3, outC channels).  Parameter names and shapes are the reference's
    state_dict keys, so `load_state_dict(dict(np.load("srnets_weights.npz")))` loads an exported model.  The nets run in
    liblerf_hip.so (lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32); `predict` is the reference's torch glue."""

    def __init__(self, opt, inC=1, outC=3):
        super(SRNetsSWF2, self).__init__()
        nf = opt.nf
        if nf != 64:
            raise NotImplementedError("only nf=64 (the shipped models) is implemented")
        self.modes2 = opt.modes2
        self.modes = opt.modes
        self.stages = opt.stages
        self.norm = opt.norm
        self.outC = outC
        for s in range(self.stages):
            if s + 1 == self.stages:
                for mode in self.modes2:
                    for r in [0, 1]:
                        self.add_module("s{}_{}r{}".format(s + 1, mode, r), _SRNet(mode, nf, outC))
            else:
                for mode in self.modes:
                    self.add_module("s{}_{}r0".format(s + 1, mode), _SRNet(mode, nf, 1))

    def forward(self, x, stage, mode, r):
        """[B, C, h+P, w+P] -> tanh of the net, [B, C*outC, h, w] (P = the mode's reach)"""
        _mode_char(mode)
        return getattr(self, "s{}_{}r{}".format(str(stage), mode, r))(x)

    _rotation_ensemble = SWF2LUT._rotation_ensemble

    def predict(self, x, stage=None):
        """x in [0, 1]; stage 2 -> hyper-parameter maps in [0, 1], otherwise the pre-filtered image in 0..255
        (model.py:101-129)."""
        half = self.norm // 2
        if stage == 2:          # hyper stage: net r0 serves rotations 0 and 2, net r1 rotations 1 and 3
            pred = self._rotation_ensemble(x, self.modes2, self.stages, lambda q: q & 1, scale=half)
            return torch.clamp(round_func(pred / (len(self.modes2) * 4) + half), 0, self.norm) / float(self.norm)
        for s in range(self.stages - 1):
            pred = self._rotation_ensemble(x, self.modes, s + 1, lambda q: 0, scale=half)
            if s + 1 == self.stages - 1:
                avg_factor, bias, norm = len(self.modes), 0, 1
            else:
                avg_factor, bias, norm = len(self.modes) * 4, half, float(self.norm)
            x = torch.clamp(round_func(pred / avg_factor) + bias, 0, self.norm) / norm
        return x


def export_srnets(model: SRNetsSWF2, exp_dir: str):
    """`<exp_dir>/srnets_weights.npz`: the model's state_dict as float32 arrays, what transfer_to_lut.load_weights reads
    (python -m lerf_pytorch_amd.resample.transfer_to_lut -e <exp_dir> then writes the LUTs)."""
    os.makedirs(exp_dir, exist_ok=True)
    path = os.path.join(exp_dir, "srnets_weights.npz")
    np.savez(path, **{k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()})
    return path


def export_luts(model: SWF2LUT, exp_dir: str, lut_name: str = "LUTft"):
    """Write the fine-tuned int8 LUTs the way train_model.py:481-497 does:
    `<exp_dir>/<lut_name>_s{stage}_{mode}r{r}.npy = round(clip(weight, -1, 1) * 127).astype(int8)` -- the files
    eval_lut_sr / eval_lut_warp (here: LutSet.from_dir, LerfEngine) load."""
    paths = []
    os.makedirs(exp_dir, exist_ok=True)
    keys = ["s2_{}r{}".format(m, r) for m in model.modes2 for r in (0, 1)] + ["s1_{}r0".format(m) for m in model.modes]
    for key in keys:
        w = getattr(model, "weight_" + key).detach().cpu().numpy()
        p = os.path.join(exp_dir, "{}_{}.npy".format(lut_name, key))
        np.save(p, np.round(np.clip(w, -1, 1) * 127).astype(np.int8))
        paths.append(p)
    return paths


def mulut_predict(model_G, x, stage=1, inC=1):
    """train_model.py:38-46: the model sees one channel at a time when inC == 1."""
    if inC == 1:
        return torch.cat([model_G.predict(x[:, i:i + 1, :, :], stage=stage) for i in range(x.shape[1])], dim=1)
    return model_G.predict(x, stage=stage)


def lutft_step(model_G, resizer, im, lb, opt_G=None, linear=False, norm=255, featC=1, reduce_grads=None, inC=1, two_stage=True):
    """One LUT fine-tuning iteration, train_model.py:416-442 (`--lutft --twoStage`): stage 1 -> stage 2 -> spatially
    varying resize -> clamp -> MSE against the HR patch; backward; optimiser step.  `resizer` is a torch-facing
    resampler with set_shape already called for im's shape.  `reduce_grads(model)` (e.g. dist.allreduce_grads) runs
    between backward and step for data-parallel training.  `inC` is the reference's opt.inC: 1 shows the model one channel
    at a time, 3 (LeRF-Net: IMDN2(opt, inC=3, outC=3), featC=3) all of them.  `two_stage=False` is the reference without
    --twoStage (:423-425): no pre-filter stage, the resampler reads round(im * norm).  Returns the loss tensor."""
    if opt_G is not None:
        opt_G.zero_grad()
    if two_stage:
        feat_im = mulut_predict(model_G, im, 1, inC)
        hyper_in = feat_im / float(norm)
    else:
        feat_im = torch.round(im * norm)
        hyper_in = im
    pred_hyper = mulut_predict(model_G, hyper_in, 2, inC)
    if linear:
        pred = resizer.resize(feat_im, pred_hyper)
    else:
        pred = resizer.resize(feat_im, pred_hyper[:, :1 * featC, :, :], pred_hyper[:, 1 * featC:2 * featC, :, :],
                              pred_hyper[:, 2 * featC:, :, :])
    pred = torch.clamp(pred, 0, norm) / float(norm)
    loss_G = F.mse_loss(pred, lb)
    if loss_G.requires_grad:
        loss_G.backward()
        if reduce_grads is not None:
            reduce_grads(model_G)
        if opt_G is not None:
            opt_G.step()
    return loss_G


# ------------------------------------------------------------------ LeRF-Net: IMDN2 (resample/model.py:434-537)
def _conv_layer(in_channels, out_channels, kernel_size):
    """model.py:435-438 conv_layer: zero padding (k-1)/2, PyTorch's default Conv2d initialisation"""
    return nn.Conv2d(in_channels, out_channels, kernel_size, 1, padding=(kernel_size - 1) // 2, bias=True)


class ShortcutBlock(nn.Module):
    def __init__(self, submodule):                               # model.py:452-459
        super(ShortcutBlock, self).__init__()
        self.sub = submodule


class IMDModule_speed(nn.Module):
    """model.py:483-508: parameter holder (c1..c5); the module runs inside lerf_imdn_fwd_f32"""

    def __init__(self, in_channels, distillation_rate=0.25):
        super(IMDModule_speed, self).__init__()
        self.distilled_channels = int(in_channels * distillation_rate)
        self.remaining_channels = int(in_channels - self.distilled_channels)
        self.c1 = _conv_layer(in_channels, in_channels, 3)
        self.c2 = _conv_layer(self.remaining_channels, in_channels, 3)
        self.c3 = _conv_layer(self.remaining_channels, in_channels, 3)
        self.c4 = _conv_layer(self.remaining_channels, self.distilled_channels, 3)
        self.act = nn.LeakyReLU(0.05, True)
        self.c5 = _conv_layer(self.distilled_channels * 4, in_channels, 1)


class _IMDNFn(torch.autograd.Function):
    """One IMDN_RTC net with its backward (lerf_imdn_fwd_train_f32 / lerf_imdn_bwd_f32); the weights arrive packed
    (torch.cat of the parameters, so autograd hands each parameter its slice of the packed gradient)."""

    @staticmethod
    def forward(ctx, flat, x, nf, in_nc, out_nc, post):
        if not (flat.is_cuda and x.is_cuda):
            raise ValueError("IMDN2 runs on the GPU (there is no CPU path)")
        w = flat.detach().contiguous().float()
        xin = x.detach().contiguous().float()
        B, _, H, W = xin.shape
        L = _lib.lib()
        nbytes = L.lerf_imdn_saved_bytes(nf, in_nc, out_nc, B, H, W)
        saved = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        out = torch.empty((B, out_nc, H, W), dtype=torch.float32, device=x.device)
        _lib.check(L.lerf_imdn_fwd_train_f32(C.c_void_p(w.data_ptr()), nf, in_nc, out_nc, C.c_void_p(xin.data_ptr()), B, H, W,
                                             int(post), C.c_void_p(saved.data_ptr()), nbytes, C.c_void_p(out.data_ptr()),
                                             _lib.current_stream()), "lerf_imdn_fwd_train_f32")
        ctx.save_for_backward(w, xin, saved)
        ctx.meta = (nf, in_nc, out_nc, int(post), nbytes)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w, x, saved = ctx.saved_tensors
        nf, in_nc, out_nc, post, nbytes = ctx.meta
        B, _, H, W = x.shape
        g = grad_out.contiguous().float()
        gw = torch.empty_like(w)                                  # overwritten, every float
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        L = _lib.lib()
        ws_bytes = L.lerf_imdn_bwd_workspace_bytes(nf, in_nc, out_nc, B, H, W)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=x.device)
        _lib.check(L.lerf_imdn_bwd_f32(C.c_void_p(w.data_ptr()), nf, in_nc, out_nc, C.c_void_p(x.data_ptr()), B, H, W, post,
                                       C.c_void_p(saved.data_ptr()), nbytes, C.c_void_p(g.data_ptr()), C.c_void_p(gw.data_ptr()),
                                       C.c_void_p(gx.data_ptr() if gx is not None else None), C.c_void_p(ws.data_ptr()), ws_bytes,
                                       _lib.current_stream()), "lerf_imdn_bwd_f32")
        return (gw if ctx.needs_input_grad[0] else None), gx, None, None, None, None


class IMDN_RTC(nn.Module):
    """model.py:512-527 at upscale 1 (the only scale IMDN2 uses): fea_conv, ShortcutBlock(5 x IMDModule_speed +
    LR_conv), upsampler conv + PixelShuffle(1).  Parameters under the reference's `model.*` keys; the net runs in
    liblerf_hip.so, on the GPU: lerf_imdn_fwd_f32 without autograd, and after enable_backward() the trainable pair
    lerf_imdn_fwd_train_f32 / lerf_imdn_bwd_f32 whenever autograd is recording."""

    def __init__(self, in_nc=3, nf=12, num_modules=5, out_nc=3, upscale=1):
        super(IMDN_RTC, self).__init__()
        if upscale != 1 or num_modules != 5:
            raise NotImplementedError("IMDN_RTC is implemented at upscale 1 with 5 modules (IMDN2's configuration)")
        self.nf, self.in_nc, self.out_nc = nf, in_nc, out_nc
        self._hip_backward = False
        rb_blocks = [IMDModule_speed(in_channels=nf) for _ in range(num_modules)]
        self.model = nn.Sequential(_conv_layer(in_nc, nf, 3), ShortcutBlock(nn.Sequential(*rb_blocks, _conv_layer(nf, nf, 1))),
                                   _conv_layer(nf, out_nc, 3), nn.PixelShuffle(1))

    def packed(self):
        """the parameters flattened in state_dict order: the packed layout of lerf_imdn_fwd_f32"""
        return torch.cat([p.detach().reshape(-1) for p in self.parameters()]).float().contiguous()

    def enable_backward(self, flag=True):
        """Opt in to (or out of) training: with it, `run` under autograd goes through lerf_imdn_fwd_train_f32 and
        lerf_imdn_bwd_f32; without it (the default) autograd is refused.  torch.no_grad() takes the inference path
        either way."""
        self._hip_backward = bool(flag)
        return self

    def run(self, x, post=0):
        """[B, in_nc, H, W] -> [B, out_nc, H, W]: the net (post 0), or predict's clamp and affine fused (1, 2)"""
        recording = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if recording and not self._hip_backward:
            raise NotImplementedError("IMDN2 refuses autograd by default: run it under torch.no_grad(), or opt in to "
                                      "training with enable_backward()")
        if not x.is_cuda:
            raise ValueError("IMDN2 runs on the GPU (there is no CPU path)")
        if x.dim() != 4 or x.shape[1] != self.in_nc:
            raise ValueError("expected [B, %d, H, W], got %s" % (self.in_nc, tuple(x.shape)))
        if recording:
            flat = torch.cat([p.reshape(-1) for p in self.parameters()])
            return _IMDNFn.apply(flat, x, self.nf, self.in_nc, self.out_nc, int(post))
        w = self.packed().to(x.device)
        xin = x.detach().contiguous().float()
        B, _, H, W = xin.shape
        L = _lib.lib()
        nbytes = L.lerf_imdn_workspace_bytes(self.nf, B, H, W)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        out = torch.empty((B, self.out_nc, H, W), dtype=torch.float32, device=x.device)
        _lib.check(L.lerf_imdn_fwd_f32(C.c_void_p(w.data_ptr()), self.nf, self.in_nc, self.out_nc, C.c_void_p(xin.data_ptr()),
                                       B, H, W, int(post), C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(out.data_ptr()),
                                       _lib.current_stream()), "lerf_imdn_fwd_f32")
        return out

    def forward(self, input):
        return self.run(input, 0)


class IMDN2(nn.Module):
    """LeRF-Net / LeRF-Net++ (model.py:530-545): stage1 in_nc -> inC, stage2 inC -> inC * outC, both IMDN_RTC nets of
    width opt.nf.  predict(x, 1) = clamp(y1, -1, 1) * (norm // 2) + norm // 2, predict(x, 2) = clamp(y2, -1, 1) / 2 + 1/2.
    Autograd is refused by default (evaluate under torch.no_grad(), as the reference's evaluation does);
    enable_backward() opts both stages in to training, e.g. lutft_step(model.enable_backward(), resizer, im, lb, opt)."""

    def __init__(self, opt, inC=1, outC=1):
        super(IMDN2, self).__init__()
        self.norm = opt.norm
        self.stage1 = IMDN_RTC(nf=opt.nf, in_nc=inC, out_nc=inC, upscale=1)
        self.stage2 = IMDN_RTC(nf=opt.nf, in_nc=inC, out_nc=inC * outC, upscale=1)

    def enable_backward(self, flag=True):
        """both stages' IMDN_RTC.enable_backward"""
        self.stage1.enable_backward(flag)
        self.stage2.enable_backward(flag)
        return self

    def predict(self, x, stage=1):
        if stage == 2:  # hyper: [0-1]
            return self.stage2.run(x, 2)
        half = self.norm // 2
        if half == 127:
            return self.stage1.run(x, 1)
        return torch.clamp(self.stage1.run(x, 0), -1, 1) * half + half


def export_imdn2(model: IMDN2, exp_dir: str):
    """`<exp_dir>/imdn2_weights.npz`: the model's state_dict as float32 arrays (what load_imdn2 and eval_model read)."""
    os.makedirs(exp_dir, exist_ok=True)
    path = os.path.join(exp_dir, "imdn2_weights.npz")
    np.savez(path, **{k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()})
    return path


def load_state(path):
    """A state dict from an exported `*_weights.npz` or from a `.pth` holding a plain state dict (a reference
    Model_XXXXXX.pth pickles the whole module: convert it once with torch.save(torch.load(p).state_dict(), q))."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k].copy()) for k in z.files}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError("%s does not hold a plain state dict" % path)
    return sd


def load_imdn2(model: IMDN2, path: str):
    """load_state_dict(strict=True) from imdn2_weights.npz or a state-dict .pth (a directory: its imdn2_weights.npz)"""
    if os.path.isdir(path):
        path = os.path.join(path, "imdn2_weights.npz")
    model.load_state_dict(load_state(path), strict=True)
    return model
