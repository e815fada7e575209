"""Gradients of one IMDN_RTC net with IMDN2.predict's clamp and affine, by torch autograd through
imdn_ref64.torch_imdn_rtc in any dtype and on any device (a helper for test_imdn_grad_cpu.py and test_gpu_imdn_train.py,
not a test).  The clamp is restated on its own: the cotangent of the raw output y is G * factor * [-1 <= y <= 1] with the
factor 127 (post 1) or 1/2 (post 2), torch.clamp's derivative, so the checker does not lean on autograd for the mask."""
import numpy as np

import imdn_ref64 as R


def net_keys(sd, prefix):
    return [k for k in sd if k.startswith(prefix)]


def net_grads(torch, sd, prefix, x, G, post, dtype, device="cpu"):
    """sd {key: float32 array}, x and G arrays -> (raw output y, {key: gradient}, grad_x) as float64 numpy arrays: the
    gradients of sum(G * post(net(x))), computed in `dtype` on `device`"""
    keys = net_keys(sd, prefix)
    sdt = {k: torch.tensor(sd[k], dtype=dtype, device=device).requires_grad_() for k in keys}
    xt = torch.tensor(np.asarray(x), dtype=dtype, device=device).requires_grad_()
    y = R.torch_imdn_rtc(sdt, prefix, xt)
    gy = torch.tensor(np.asarray(G), dtype=dtype, device=device)
    if post:
        yd = y.detach()
        gy = gy * (127.0 if post == 1 else 0.5) * ((yd >= -1) & (yd <= 1)).to(dtype)
    y.backward(gy)
    to64 = lambda t: t.detach().double().cpu().numpy()
    return to64(y), {k: to64(sdt[k].grad) for k in keys}, to64(xt.grad)


def rel_err(t, t64):
    """max |t - t64| / max |t64|"""
    return float(np.abs(np.asarray(t, np.float64) - t64).max() / max(np.abs(t64).max(), 1e-300))
